// Device code of the block ingest, shared by ingest.hip's kernels and
// the online committee verify (comb.hip's k_verify_comb16, which ingests its own blocks). The
// walk is bincode_walk.h's, the rules block_verdict.h's; the references are ingest.hip's header
// comment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "bincode_walk.h"
#include "block_verdict.h"
#include "ingest_lane.h"

namespace mv {

// ---------------------------------------------------------------- wave per block
// k_block_ingest: one 64-lane workgroup per block. The block's bincode is staged in LDS with
// coalesced 8-byte loads; the fixed-size includes are transcoded one per lane; the
// variable-size statements are located 64 at a time by lane 0 walking their headers, then
// transcoded one per lane (Share payloads copied by the whole wave); the pre-image is built
// in LDS and written to the stage with coalesced stores. Blocks that do not fit the LDS
// window take the one-lane function ingest_lane on lane 0. The rules are the shared walk's
// (bincode_walk.h), block_verdict.h's and block_codec.cpp's; tests/test_gpu_ingest.py holds every ingest form and the host codec to
// identical results.
constexpr uint32_t IG_WIN = 10240;  // LDS window per block, bytes
constexpr uint32_t IG_CHUNK = 64;   // statements located per walk

MV_DEV uint32_t lds_u8(const uint32_t* w, uint32_t p) { return (w[p >> 2] >> (8 * (p & 3))) & 0xffu; }
MV_DEV uint32_t lds_u32(const uint32_t* w, uint32_t p) {
  const uint32_t i = p >> 2, sh = (p & 3) * 8;
  return __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
}
MV_DEV uint64_t lds_u64(const uint32_t* w, uint32_t p) {
  const uint32_t i = p >> 2, sh = (p & 3) * 8;
  const uint32_t x0 = w[i], x1 = w[i + 1], x2 = w[i + 2];
  return ((uint64_t)__builtin_amdgcn_alignbit(x2, x1, sh) << 32) | __builtin_amdgcn_alignbit(x1, x0, sh);
}
MV_DEV void pre_be64(uint8_t* pre, uint32_t p, uint64_t x) {
#pragma unroll
  for (int b = 0; b < 8; b++) pre[p + b] = (uint8_t)(x >> (56 - 8 * b));
}
// 32 bytes of the window at byte q (any alignment): the 9 covering words, read together
MV_DEV void win_read32(uint32_t w[9], const uint32_t* win, uint32_t q) {
  const uint32_t i = q >> 2;
#pragma unroll
  for (int k = 0; k < 9; k++) w[k] = win[i + k];
}
// ... written to the pre-image at p (q = the byte address they were read from)
MV_DEV void pre_write32(uint8_t* pre, uint32_t p, const uint32_t w[9], uint32_t q) {
  const uint32_t sh = (q & 3) * 8;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t x = __builtin_amdgcn_alignbit(w[k + 1], w[k], sh);
#pragma unroll
    for (int b = 0; b < 4; b++) pre[p + 4 * k + b] = (uint8_t)(x >> (8 * b));
  }
}
MV_DEV uint32_t wave_min(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, m));
  return x;
}
MV_DEV uint32_t wave_or(uint32_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x |= (uint32_t)__shfl_xor((int)x, m);
  return x;
}
MV_DEV uint64_t wave_sum64(uint64_t x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), m);
    x += ((uint64_t)hi << 32) | lo;
  }
  return x;
}

// The LDS a wave needs to ingest one block.
struct IngestLds {
  uint64_t win64[IG_WIN / 8 + 4];
  uint32_t st_pos[IG_CHUNK], st_pre[IG_CHUNK];
  uint32_t seen[16];  // authorities of round r-1 among the includes
};
template <bool WAVE>
MV_DEV void ig_sync() {
  if (WAVE) {  // one wave of a larger workgroup (k_verify_comb16): wave-scope ordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// Block i by one wave (k_block_ingest's body; WAVE: the wave is one of several in its
// workgroup and syncs alone). L: the wave's own LDS.
template <bool WAVE>
MV_DEV void ingest_block(uint32_t i, const uint8_t* __restrict__ buf, const uint64_t* __restrict__ off,
                         const uint64_t* __restrict__ len, const CommitteeView& cv, const IngestOut& io,
                         IngestLds& Ls) {
  uint64_t* win64 = Ls.win64;
  uint32_t* st_pos = Ls.st_pos;
  uint32_t* st_pre = Ls.st_pre;
  uint32_t* seen = Ls.seen;
  // The block's bincode (from its aligned start), transcoded IN PLACE into its pre-image ||
  // signature: every element's pre-image starts at or before its bincode and the elements
  // are produced in order, so an element's pre-image never reaches bincode not yet read
  // (each chunk's lanes read their elements into registers before any of them writes). One
  // 10-KB buffer instead of two doubles the waves per CU (LDS-limited, 7 -> 14).
  uint32_t* win = reinterpret_cast<uint32_t*>(win64);
  uint64_t* pre64 = win64;
  uint8_t* pre = reinterpret_cast<uint8_t*>(win64);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t o = off[i], L = len[i];
  const uint32_t d = (uint32_t)(o & 7);
  if (lane < 16) seen[lane] = 0;
  if (d + L + 16 > IG_WIN) {  // does not fit the window: one lane from global memory
    ig_sync<WAVE>();
    if (lane == 0) ingest_lane(buf, o, L, i, cv, io, seen, 1);
    return;
  }
  {
    // every load of the window in flight at once (IG_LOADS per lane) before the LDS stores:
    // a store right behind each load would serialise the HBM latency 19 times for a 9.5-KB
    // block, and 16 per lane still took two rounds for it. The fit test above bounds nw by
    // IG_WIN / 8 = 64 * IG_LOADS, so one round always covers the block.
    constexpr int IG_LOADS = IG_WIN / 8 / 64;
    static_assert(IG_WIN % 512 == 0, "the window is whole 64-lane rounds of 8-byte loads");
    const uint64_t* src = reinterpret_cast<const uint64_t*>(buf + (o - d));
    uint64_t* w64 = win64;
    const uint32_t nw = (uint32_t)((d + L + 15) >> 3);
    uint64_t t[IG_LOADS];
#pragma unroll
    for (int j = 0; j < IG_LOADS; j++) t[j] = lane + 64 * j < nw ? src[lane + 64 * j] : 0ull;
#pragma unroll
    for (int j = 0; j < IG_LOADS; j++)
      if (lane + 64 * j < nw) w64[lane + 64 * j] = t[j];
  }
  ig_sync<WAVE>();
  const uint32_t Lb = (uint32_t)L;
  auto rd64 = [&](uint32_t p) { return lds_u64(win, d + p); };
  auto rd32 = [&](uint32_t p) { return lds_u32(win, d + p); };
  auto rd8 = [&](uint32_t p) { return lds_u8(win, d + p); };
  const uint32_t n_auth = cv.n_auth;

  // reference (56 B) and the include count
  bool ok = Lb >= 64;
  uint64_t me_a = 0, me_r = 0;
  if (ok) {
    me_a = rd64(0);
    me_r = rd64(8);
    ok = rd64(16) == 32;
  }
  const uint64_t n_inc = ok ? rd64(56) : 0;
  if (ok && n_inc > (uint64_t)((Lb - 64) / 56)) ok = false;
  // the claimed digest (bincode bytes 24..56), one word per lane 0..7, before the includes'
  // pre-images overwrite it
  const uint32_t claimed_w = (ok && lane < 8) ? rd32(24 + 4 * lane) : 0u;
  uint32_t bad = 0, inc_first = 0xffffffffu;
  if (ok) {
    if (lane < 8) {
      pre[lane] = (uint8_t)(me_a >> (56 - 8 * lane));
      pre[8 + lane] = (uint8_t)(me_r >> (56 - 8 * lane));
    }
    // includes: lane per include (pre-image at 16 + 48 k), checks (types.rs:349-362),
    // the threshold clock's authorities of round r-1 (threshold_clock.rs:12-35)
    for (uint32_t k = lane; k < (uint32_t)n_inc; k += 64) {
      const uint32_t p = 64 + 56 * k;
      const uint64_t a = rd64(p), r = rd64(p + 8);
      bad |= rd64(p + 16) != 32;
      uint64_t dg[4];
#pragma unroll
      for (int m = 0; m < 4; m++) dg[m] = rd64(p + 24 + 8 * m);  // digest bytes as they lie
      // pre-image offset 16 + 48 k is 8-byte aligned: six 64-bit LDS stores, not 48 byte stores
      uint64_t* pq = pre64 + 2 + 6 * k;
      pq[0] = __builtin_bswap64(a);  // big-endian u64 (pre_be64)
      pq[1] = __builtin_bswap64(r);
#pragma unroll
      for (int m = 0; m < 4; m++) pq[2 + m] = dg[m];
      const uint32_t code = include_code(a, r, me_r, n_auth);
      if (code && inc_first == 0xffffffffu) inc_first = (k << 4) | code;
      if (clock_include(a, r, me_r, n_auth)) atomicOr(&seen[(uint32_t)a >> 5], 1u << (a & 31));
    }
  }
  inc_first = wave_min(inc_first);
  // statements: located by lane 0 (headers only), 64 at a time, then transcoded per lane
  uint32_t pos = 64 + 56 * (uint32_t)n_inc, ppos = 16 + 48 * (uint32_t)n_inc;
  uint64_t n_st = 0;
  if (ok) {
    if (pos + 8 > Lb) ok = false;
    else n_st = rd64(pos);
    pos += 8;
  }
  uint32_t vr_first = 0xffffffffu;  // (statement index << 2) | vr_code of the first failing range
  for (uint64_t k0 = 0; ok && k0 < n_st; k0 += IG_CHUNK) {
    // Locate up to IG_CHUNK statements. Speculation: lane j assumes the j statements
    // before it are VoteRanges (76 B in bincode, 65 in the pre-image) and checks its own
    // tag; the run of confirmed VoteRanges is taken at once, anything else takes one
    // scalar step (the whole wave computes it identically).
    uint32_t c = 0, p = pos, pp = ppos;
    bool lok = true;
    while (c < IG_CHUNK && k0 + c < n_st) {
      const uint32_t j = c + lane;
      const uint32_t q = p + 76 * lane;
      const bool rng = j < IG_CHUNK && k0 + j < n_st && q + 76 <= Lb && rd32(q) == 2;
      const uint64_t brk = __ballot(!rng);
      const uint32_t run = brk ? (uint32_t)__builtin_ctzll(brk) : 64u;
      if (lane < run) {
        st_pos[j] = q;
        st_pre[j] = pp + 65 * lane;
      }
      c += run;
      p += 76 * run;
      pp += 65 * run;
      if (c >= IG_CHUNK || k0 + c >= n_st) break;
      uint32_t size = 0, psize = 0;
      if (p + 4 > Lb) { lok = false; break; }
      const uint32_t tag = rd32(p);
      if (tag == 0) {  // Share: u32 tag, u64 length, bytes
        if (p + 12 > Lb) { lok = false; break; }
        const uint64_t l = rd64(p + 4);
        if (l > (uint64_t)(Lb - p - 12)) { lok = false; break; }
        size = 12 + (uint32_t)l;
        psize = 1 + (uint32_t)l;
      } else if (tag == 1) {  // Vote: locator (64 B), u32 vote, [u8 option, [locator]]
        if (p + 72 > Lb) { lok = false; break; }
        const uint32_t vote = rd32(p + 68);
        if (vote == 0) {
          size = 72;
          psize = 57;
        } else if (vote == 1 && p + 73 <= Lb) {
          const uint32_t some = rd8(p + 72);
          if (some == 0) {
            size = 73;
            psize = 57;
          } else if (some == 1 && p + 137 <= Lb) {
            size = 137;
            psize = 113;
          } else {
            lok = false;
            break;
          }
        } else {
          lok = false;
          break;
        }
      } else {  // tag 2 here means a truncated VoteRange; others are invalid
        lok = false;
        break;
      }
      if (lane == 0) {
        st_pos[c] = p;
        st_pre[c] = pp;
      }
      c++;
      p += size;
      pp += psize;
    }
    ig_sync<WAVE>();
    const uint32_t cnt = c;
    ok = lok;
    // (a) every lane reads its statement into registers
    uint32_t kind = 0;  // 1 Share, 2 Accept, 3 Reject(None), 4 Reject(Some), 5 VoteRange
    uint32_t q = 0, ps = 0;
    uint64_t a = 0, r = 0, x = 0, y = 0, a2 = 0, r2 = 0, z2 = 0;
    uint32_t dg[9], dg2[9];
    if (lane < cnt) {
      const uint32_t p = st_pos[lane];
      q = st_pre[lane];
      ps = p;
      const uint32_t tag = rd32(p);
      if (tag == 0) {
        kind = 1;
      } else {
        a = rd64(p + 4);
        r = rd64(p + 12);
        bad |= rd64(p + 20) != 32;
        win_read32(dg, win, d + p + 28);
        x = rd64(p + 60);
        if (tag == 1) {
          const uint32_t vote = rd32(p + 68);
          const uint32_t some = vote == 1 ? rd8(p + 72) : 0u;
          kind = vote == 0 ? 2 : (some == 0 ? 3 : 4);
          if (kind == 4) {
            a2 = rd64(p + 73);
            r2 = rd64(p + 81);
            bad |= rd64(p + 89) != 32;
            win_read32(dg2, win, d + p + 97);
            z2 = rd64(p + 129);
          }
        } else {  // tag 2
          kind = 5;
          y = rd64(p + 68);
          const uint32_t code = vr_code(x, y);
          if (code && vr_first == 0xffffffffu) vr_first = ((uint32_t)(k0 + lane) << 2) | code;
        }
      }
    }
    // (b) Share payloads, moved down by the whole wave 64 bytes at a time (each round reads
    // before it writes, and the destination lies below the source)
    uint64_t shares = __ballot(kind == 1);
    while (shares) {
      const uint32_t j = (uint32_t)__builtin_ctzll(shares);
      shares &= shares - 1;
      const uint32_t p = st_pos[j], qj = st_pre[j];
      const uint32_t l = (uint32_t)rd64(p + 4);
      for (uint32_t t = lane; t < ((l + 63) & ~63u); t += 64) {
        const uint32_t v = t < l ? rd8(p + 12 + t) : 0u;
        if (t < l) pre[qj + 1 + t] = (uint8_t)v;
      }
    }
    // (c) every lane writes its statement's pre-image
    if (kind == 1) {
      pre[q] = 0;
    } else if (kind >= 2 && kind <= 4) {
      pre[q] = (uint8_t)(kind - 1);
      pre_be64(pre, q + 1, a);
      pre_be64(pre, q + 9, r);
      pre_write32(pre, q + 17, dg, d + ps + 28);
      pre_be64(pre, q + 49, x);
      if (kind == 4) {
        pre_be64(pre, q + 57, a2);
        pre_be64(pre, q + 65, r2);
        pre_write32(pre, q + 73, dg2, d + ps + 97);
        pre_be64(pre, q + 105, z2);
      }
    } else if (kind == 5) {
      pre[q] = 4;
      pre_be64(pre, q + 1, a);
      pre_be64(pre, q + 9, r);
      pre_write32(pre, q + 17, dg, d + ps + 28);
      pre_be64(pre, q + 49, x);
      pre_be64(pre, q + 57, y);
    }
    pos = p;
    ppos = pp;
    ig_sync<WAVE>();  // st_* are rewritten by the next chunk
  }
  // meta_creation_time_ns (u128 LE), epoch_marker (bool), epoch, signature (u64 64 + 64 B)
  uint64_t tlo = 0, thi = 0, ep = 0;
  uint32_t marker = 0;
  if (ok) {
    if (pos + 97 > Lb) {
      ok = false;
    } else {
      tlo = rd64(pos);
      thi = rd64(pos + 8);
      marker = rd8(pos + 16);
      ep = rd64(pos + 17);
      ok = marker <= 1 && rd64(pos + 25) == 64;
    }
  }
  ok = ok && wave_or(bad) == 0;
  const uint32_t spos = pos + 33;  // signature
  uint32_t f = 0;
  if (ok) {
    if (lane == 0) {
      pre_be64(pre, ppos, thi);
      pre_be64(pre, ppos + 8, tlo);
      pre[ppos + 16] = (uint8_t)marker;
      pre_be64(pre, ppos + 17, ep);
    }
    const uint32_t sb = rd8(spos + lane);  // P || sig (read by every lane before any writes)
    pre[ppos + 25 + lane] = (uint8_t)sb;
    // threshold clock: stake of the distinct round r-1 authorities among the includes
    // (lane j sums authorities j, j + 64, ...: independent loads, one latency)
    uint64_t stake = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
      const uint32_t a = lane + 64 * q;
      if (a < n_auth && ((seen[a >> 5] >> (a & 31)) & 1u)) stake += cv.stakes[a];
    }
    stake = wave_sum64(stake);
    const uint32_t inc_code = inc_first == 0xffffffffu ? 0u : (inc_first & 15u);
    vr_first = wave_min(vr_first);
    const uint32_t vr = vr_first == 0xffffffffu ? 0u : (vr_first & 3u);
    f = block_facts(ep == cv.epoch, me_a < n_auth, me_r == 0, vr, stake > cv.quorum_thr, inc_code);
  }
  ig_sync<WAVE>();
  const uint64_t so = (o + 7) & ~7ull;
  const uint32_t plen = ppos + 25;
  if (ok) {  // P || sig to the stage (it stays inside the block's own span, see ingest_lane)
    uint64_t* dst = reinterpret_cast<uint64_t*>(io.stage + so);
    const uint32_t nw = (plen + 64 + 7) >> 3;
    for (uint32_t k = lane; k < nw; k += 64) dst[k] = pre64[k];
  }
  if (ok && lane < 8) reinterpret_cast<uint32_t*>(io.claimed + 32 * (size_t)i)[lane] = claimed_w;
  if (lane == 0) {
    io.pre_off[i] = so;
    io.pre_len[i] = ok ? plen : 0;
    uint32_t sw[16];  // the signature, from its pre-image copy (its bincode was overwritten)
#pragma unroll
    for (int q = 0; q < 16; q++) sw[q] = ok ? lds_u32(win, plen + 4 * q) : 0u;
    store_sig(io.sig_out, i, sw, f);
    io.key_idx[i] = block_key(f, (uint32_t)me_a);
    io.facts[i] = f;
  }
}

}  // namespace mv
