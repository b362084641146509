// WAL replay check on gfx950: crc32fast::hash (CRC-32/ISO-HDLC) of
// every WAL entry's payload, and the entry walk of WalIterator (mysticeti-core/src/wal.rs:
// 226-346) over a WAL image in HBM.
//
// CRC: one wave per byte string D = [a, b). The string is cut into rows of 256 bytes that
// END at b (the first row is padded in front); lane l owns 32-bit word l of every row and
// folds its words by Horner with the linear map "advance 256 bytes":
//     u_l <- A256(u_l) ^ w_{l,j}
// so u_l = XOR_j shift(w_{l,j}, 256 (R-1-j)). The lanes then combine in a 6-level tree
// (shifts by 4, 8, ..., 128 bytes) and a final 4-byte shift. Every shift is a GF(2)-linear
// map applied as four 256-entry table lookups (one per state byte). The initial value
// 0xFFFFFFFF is folded in as a 4-byte prefix P with crc_raw(0, P) = 0xFFFFFFFF placed just
// before a (zeros before it change nothing from state 0), so no per-string variable shift
// is needed. Unaligned b: each lane reads the two aligned dwords around its word and
// funnel-shifts them (v_alignbyte_b32).
// Tables in LDS: A256 (the hot one, 4 x 256 words) replicated 8 times so that lanes l and
// l' with l != l' (mod 8) never hit one bank; the tree's six maps once (56 KiB in all, one
// copy per 1024-thread workgroup, two workgroups per CU). The kernel is bound by HBM latency,
// not by the LDS: 32 bank-aligned copies (no conflicts at all, 152 KiB, one workgroup per CU)
// measured 3.18 ms per 2^20 entries and 16 copies 2.52, against 2.31 for this form at 8 waves
// per SIMD (profiles/r04/wal/ab_tables_occupancy_r04p.txt).
//
// Walk: one lane per map of 2^map_bits bytes. Every map that holds entries starts with one
// (the writer pads an entry that would straddle a map, wal.rs:155-167), so maps walk
// independently; the host then joins them in the reference's iteration order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "kernels.h"
#include "wal_crc.h"

namespace mv {
namespace wal {

// ------------------------------------------------------------------ crc32 of n strings
__global__ void __launch_bounds__(WG) MV_WAL_ATTR k_crc32_batch(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ len, uint32_t n,
                                                    const uint32_t* __restrict__ tables, uint32_t* __restrict__ out) {
  __shared__ Lds L;
  lds_fill(L, tables);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (WG / 64);
  for (uint32_t i = blockIdx.x * (WG / 64) + threadIdx.x / 64; i < n; i += waves) {
    const uint64_t a = bcast64(off[i]), b = a + bcast64(len[i]);
    const uint32_t r = crc_raw_wave(buf, a, b, L, s_tab(L, tables));
    if (lane == 0) out[i] = ~r;
  }
}

// ------------------------------------------------------------------ WAL walk
// map flags (the iteration after this map's entries)
// EMPTY: no entry at the map start, the iteration ends before the map; NEXT: it continues at
// the next map's start; END: it reached end_pos; BAD: the last record failed (a reference panic)
constexpr uint8_t MAP_EMPTY = mvk::WAL_MAP_EMPTY, MAP_NEXT = mvk::WAL_MAP_NEXT, MAP_END = mvk::WAL_MAP_END,
                  MAP_BAD = mvk::WAL_MAP_BAD;

MV_DEV uint64_t le64_bounded(const uint8_t* img, uint64_t size, uint64_t p) {
  if (p + 8 <= size) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(img + (p & ~3ull));
    const uint32_t s = (uint32_t)(p & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = s ? w[2] : 0u;
    const uint32_t lo = s ? __builtin_amdgcn_alignbyte(w1, w0, s) : w0;
    const uint32_t hi = s ? __builtin_amdgcn_alignbyte(w2, w1, s) : w1;
    return ((uint64_t)hi << 32) | lo;
  }
  uint64_t v = 0;
  for (int k = 7; k >= 0; k--) v = (v << 8) | (p + k < size ? img[p + k] : 0u);
  return v;
}

// record = position | status << 60 (status: MV_WAL_OK for an entry whose crc is still to check)
// The walk is a chain of dependent header reads (~1 us of HBM latency each, ~1,800 per 16-MiB map
// of config-4 blocks). It runs ahead speculatively: the headers at p + k * stride, k < WALK_AHEAD,
// are loaded together, stride = the last entry's length (WAL entries of one kind share a length);
// they are then consumed in order while each entry's length equals the stride, and the walk
// re-aims at the first that differs. The checks, records and flags are those of the one-at-a-time
// walk (wal.rs:285-346) in the same order; a mispredicted header is never used.
constexpr int WALK_AHEAD = 8;
// a header's 16 bytes at q as five aligned dwords, loaded without a branch (so the run-ahead
// loads are all in flight together); `fast` false (the header would reach past the image, or the
// image is shorter than 20 bytes): the consumer reads it byte-wise (le64_bounded)
struct WalkHdr {
  uint32_t w[5];
  bool fast;
};
MV_DEV void hdr_load(WalkHdr& h, const uint8_t* img, uint64_t size, uint64_t q) {
  h.fast = size >= 20 && q <= size - 20;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img + (h.fast ? (q & ~3ull) : 0ull));
#pragma unroll
  for (int i = 0; i < 5; i++) h.w[i] = w[i];
}
MV_DEV void hdr_get(const WalkHdr& h, const uint8_t* img, uint64_t size, uint64_t q, uint64_t& crc, uint64_t& hi) {
  if (h.fast) {
    const uint32_t s = (uint32_t)(q & 3);
    auto fn = [&](int i) { return s ? __builtin_amdgcn_alignbyte(h.w[i + 1], h.w[i], s) : h.w[i]; };
    crc = ((uint64_t)fn(1) << 32) | fn(0);
    hi = ((uint64_t)fn(3) << 32) | fn(2);
  } else {
    crc = le64_bounded(img, size, q);
    hi = le64_bounded(img, size, q + 8);
  }
}
__global__ void __launch_bounds__(64) k_wal_walk(const uint8_t* __restrict__ img, uint64_t size, uint64_t end_pos,
                                                 uint32_t map_bits, uint32_t nmaps, uint32_t cap_pm,
                                                 const uint64_t* __restrict__ moff,
                                                 unsigned long long* __restrict__ rec, uint32_t* __restrict__ mcount,
                                                 uint8_t* __restrict__ mflag) {
  const uint32_t m = blockIdx.x * 64 + threadIdx.x;
  if (m >= nmaps) return;
  const uint64_t msize = 1ull << map_bits, start = (uint64_t)m << map_bits;
  uint64_t p = start, stride = 0;
  uint32_t count = 0;
  uint8_t flag = MAP_NEXT;
  // moff (the second walk): map m's records at rec + moff[m], as many as the first walk counted
  unsigned long long* r = moff ? rec + moff[m] : rec + (size_t)m * cap_pm;
  if (moff) cap_pm = mcount[m];
  bool done = false, have_next = false;
  WalkHdr hd[WALK_AHEAD], hn[WALK_AHEAD];
  while (!done) {
    if (have_next) {
#pragma unroll
      for (int k = 0; k < WALK_AHEAD; k++) hd[k] = hn[k];
    } else {
#pragma unroll
      for (int k = 0; k < WALK_AHEAD; k++) hdr_load(hd[k], img, size, p + (uint64_t)k * stride);
    }
    const int ahead = stride ? WALK_AHEAD : 1;
    // the round after this one, in flight while this one is consumed (it is used only if all of
    // this round's entries have the stride)
    have_next = stride != 0;
    if (have_next) {
#pragma unroll
      for (int k = 0; k < WALK_AHEAD; k++) hdr_load(hn[k], img, size, p + (uint64_t)(WALK_AHEAD + k) * stride);
    }
#pragma unroll
    for (int k = 0; k < WALK_AHEAD; k++) {
      if (k >= ahead) break;
      // the entry at p (= the k-th speculative position: the lengths so far equal the stride)
      if (p >= end_pos) {
        flag = p == start ? MAP_EMPTY : MAP_END;
        done = true;
        break;
      }
      const uint64_t boff = p - start;
      if (msize - boff < 16) {  // no room for a header (wal.rs:297-300)
        flag = MAP_NEXT;
        done = true;
        break;
      }
      uint64_t crc, hi;
      hdr_get(hd[k], img, size, p, crc, hi);
      const uint64_t len = hi & 0xffffffffull;
      if (len == 0) {
        if (crc == 0) {
          flag = boff == 0 ? MAP_EMPTY : MAP_NEXT;
        } else {
          if (count < cap_pm) r[count] = p | ((unsigned long long)MV_WAL_NONZERO_CRC_LEN0 << 60);
          count++;
          flag = MAP_BAD;
        }
        done = true;
        break;
      }
      if (len < 16 || boff + len > msize) {
        if (count < cap_pm) r[count] = p | ((unsigned long long)MV_WAL_BAD_LENGTH << 60);
        count++;
        flag = MAP_BAD;
        done = true;
        break;
      }
      if (count < cap_pm) r[count] = p;
      count++;
      p += len;
      if (len != stride) {  // the next speculative header is not at p: re-aim
        stride = len;
        have_next = false;
        break;
      }
    }
  }
  mcount[m] = count;
  mflag[m] = flag;
}

// records of map m -> entries [moff[m], moff[m] + mcount[m])
__global__ void __launch_bounds__(256) k_wal_compact(const unsigned long long* __restrict__ rec, uint32_t cap_pm,
                                                     const uint32_t* __restrict__ mcount,
                                                     const uint64_t* __restrict__ moff,
                                                     unsigned long long* __restrict__ ent) {
  const uint32_t m = blockIdx.x;
  const uint32_t c = mcount[m];
  const uint64_t o = moff[m];
  for (uint32_t i = threadIdx.x; i < c; i += 256) ent[o + i] = rec[(size_t)m * cap_pm + i];
}

// one wave per entry: header, crc of the payload, verdict; the first failing entry index
// goes to *first_fail (atomic min)
__global__ void __launch_bounds__(WG) MV_WAL_ATTR k_wal_crc(const uint8_t* __restrict__ img, uint64_t size,
                                                const unsigned long long* __restrict__ ent, uint64_t total,
                                                const uint32_t* __restrict__ tables, uint64_t* __restrict__ out_pos,
                                                uint32_t* __restrict__ out_tag, uint32_t* __restrict__ out_len,
                                                uint8_t* __restrict__ out_status, uint64_t cap,
                                                unsigned long long* __restrict__ first_fail) {
  __shared__ Lds L;
  lds_fill(L, tables);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (WG / 64);
  const uint32_t* tbyte = tables + A_WORDS + S_WORDS;
  const uint32_t* S = s_tab(L, tables);
  for (uint64_t e = blockIdx.x * (WG / 64) + threadIdx.x / 64; e < total; e += waves) {
    const uint64_t r = bcast64(ent[e]);
    const uint64_t p = r & ((1ull << 60) - 1);
    uint32_t st = (uint32_t)(r >> 60);
    const uint64_t crc = bcast64(le64_bounded(img, size, p)), hi = bcast64(le64_bounded(img, size, p + 8));
    const uint64_t len = hi & 0xffffffffull;
    const uint32_t tag = (uint32_t)(hi >> 32);
    uint32_t plen = 0;
    if (st == MV_WAL_OK) {
      plen = (uint32_t)(len - 16);
      const uint64_t a = p + 16, b = p + len;
      uint32_t raw;
      if (b <= size) {
        raw = crc_raw_wave(img, a, b, L, S);
      } else {  // the file ends inside the payload: the rest reads as zeros
        raw = a < size ? crc_raw_wave(img, a, size, L, S) : 0xffffffffu;
        raw = zeros_shift(L, S, tbyte, raw, b - (a < size ? size : a));
      }
      st = (uint64_t)(~raw) == crc ? MV_WAL_OK : MV_WAL_CRC_MISMATCH;
    }
    if (lane == 0) {
      if (e < cap) {
        out_pos[e] = p;
        out_tag[e] = tag;
        out_len[e] = plen;
        out_status[e] = (uint8_t)st;
      }
      if (st != MV_WAL_OK) atomicMin(first_fail, (unsigned long long)e);
    }
  }
}

}  // namespace wal
}  // namespace mv

namespace mvk {

size_t wal_table_words() { return mv::wal::A_WORDS + mv::wal::S_WORDS + mv::wal::T_WORDS; }

// host: A256 (replicated), the tree shifts, the byte table
void wal_build_tables(uint32_t* out) {
  using namespace mv::wal;
  uint32_t T[256];
  for (uint32_t b = 0; b < 256; b++) {
    uint32_t c = b;
    for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    T[b] = c;
  }
  auto shift = [&](uint32_t s, int n) {
    for (int i = 0; i < n; i++) s = (s >> 8) ^ T[s & 255];
    return s;
  };
  for (int t = 0; t < 4; t++)
    for (int e = 0; e < 256; e++) {
      const uint32_t v = shift((uint32_t)e << (8 * t), 256);
      for (int c = 0; c < REP; c++) out[(t * 256 + e) * REP + c] = v;
    }
  for (int k = 0; k < S_LEVELS; k++)
    for (int t = 0; t < 4; t++)
      for (int e = 0; e < 256; e++) out[A_WORDS + k * 1024 + t * 256 + e] = shift((uint32_t)e << (8 * t), 4 << k);
  for (int e = 0; e < 256; e++) out[A_WORDS + S_WORDS + e] = T[e];
}

using mv::wal::crc_grid;

hipError_t launch_crc32(const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                        const uint32_t* tables, uint32_t* out, int cus, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::wal::k_crc32_batch, dim3(crc_grid(n, cus)), dim3(mv::wal::WG), 0, s, buf, off, len, n,
                     tables, out);
  return hipGetLastError();
}

hipError_t launch_wal_walk(const uint8_t* img, uint64_t size, uint64_t end_pos, uint32_t map_bits, uint32_t nmaps,
                           uint32_t cap_pm, const uint64_t* moff, unsigned long long* rec, uint32_t* mcount,
                           uint8_t* mflag, hipStream_t s) {
  if (nmaps == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::wal::k_wal_walk, dim3((nmaps + 63) / 64), dim3(64), 0, s, img, size, end_pos, map_bits, nmaps,
                     cap_pm, moff, rec, mcount, mflag);
  return hipGetLastError();
}

hipError_t launch_wal_compact(const unsigned long long* rec, uint32_t cap_pm, const uint32_t* mcount,
                              const uint64_t* moff, uint32_t nmaps, unsigned long long* ent, hipStream_t s) {
  if (nmaps == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::wal::k_wal_compact, dim3(nmaps), dim3(256), 0, s, rec, cap_pm, mcount, moff, ent);
  return hipGetLastError();
}

hipError_t launch_wal_crc(const uint8_t* img, uint64_t size, const unsigned long long* ent, uint64_t total,
                          const uint32_t* tables, uint64_t* out_pos, uint32_t* out_tag, uint32_t* out_len,
                          uint8_t* out_status, uint64_t cap, unsigned long long* first_fail, int cus, hipStream_t s) {
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::wal::k_wal_crc, dim3(crc_grid(total, cus)), dim3(mv::wal::WG), 0, s, img, size, ent, total,
                     tables, out_pos, out_tag, out_len, out_status, cap, first_fail);
  return hipGetLastError();
}

}  // namespace mvk
