// mv_wal_write on gfx950: WalWriter::writev (mysticeti-core/src/wal.rs:150-188) for n entries at
// once -- where every entry goes, then its zero gap, header and body, with the crc32 of the body
// taken in the same pass that copies it. The inverse of wal.hip's walk and crc check.
//
// Layout (rule and argument: wal_layout.h). Four launches:
//   k_compact_count / k_ix_scan / k_compact_list<LenScan>  the checks of every entry and S(i), the
//                 exclusive sums of the entry lengths (index_dev.h's pass; the total is S(n))
//   k_ww_cross    one wave: the map crossings one after another, each one wl::cross_step whose
//                 search runs on all 64 lanes (first_above); writes the step table and the end
//   k_ww_pos      one lane per entry: pos[i] = start + shift_at(i) + S(i)
// A crossing costs one to four dependent rounds of 64 loads: the first round probes 64 entries
// around the place the mean entry length predicts, which is where entries of one kind are.
// The crossings are a serial chain on one wave: span / 2^map_bits steps, a handful at the production
// map size, about one per entry at map_bits 8 (test sizes); include/mysti_verify.h states the bound.
//
// Bytes: k_ww_emit, one wave per entry, a persistent grid with the crc tables in LDS (wal_crc.h, as
// k_wal_crc). Source and destination bytes have independent alignments, so the fold's word grid is
// laid on the DESTINATION: it ends at the last 4-byte boundary of `out` inside the body. Every
// word the fold builds from the two aligned source dwords around it (v_alignbyte_b32) is then one
// aligned dword store; the one word that holds the body's first bytes is stored byte by byte, and
// the at most three bytes behind the grid are read, stored and folded one by one through the byte
// table. The payload is read once. Header (16 lanes) and next_entry (8 lanes) are byte stores: an
// entry starts at any byte, and neighbouring entries share aligned words, which no wave may
// write as a whole.
// An own block's body is next_entry's eight bytes and then the payload, which are not adjacent in
// the source: the crc register is affine in its start value, crc_raw(s, D) = crc_raw(~0, D) ^
// A^|D| (s ^ ~0), so the payload is folded from ~0 as ever and the state after the eight head
// bytes joins through zeros_shift.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "index_dev.h"
#include "kernels.h"
#include "wal_crc.h"
#include "wal_layout.h"

namespace mv {
namespace ww {

using mvk::WalWriteCall;
using namespace mv::wal;
typedef unsigned long long u64;
// The byte pass keeps the fold's eight rows in flight and, next to the fold's registers, a store
// address per row. Compiled for the 64 VGPRs of 8 waves per SIMD (k_wal_crc's budget) it spills, so
// it is cut for 4 waves per SIMD -- one 1024-thread workgroup per CU -- where it has no scratch.
#define MV_WW_ATTR __attribute__((amdgpu_waves_per_eu(4)))

// an entry's length as the scan takes it: a refused entry counts as a bare header, so that the sums
// stay below 2^64 and the crossing loop ends; the call is refused before anything reads them
__device__ inline uint64_t entry_len(const WalWriteCall& c, uint64_t i, bool* ok) {
  const uint64_t* e = c.entries + wl::ENTRY_WORDS * i;
  *ok = wl::entry_ok(e[0], e[1], e[2], c.buf_bytes, c.map_bits);
  return wl::HEADER + (*ok ? wl::body_len(e[0], e[2]) : 0);
}

struct LenScan {
  static constexpr int WEIGHTS = 1;
  WalWriteCall c;
  u64* ctl;
  __device__ void weigh(uint64_t i, uint64_t* a) const {
    bool ok;
    *a = i < c.n ? entry_len(c, i, &ok) : 0;
  }
  __device__ void place(uint64_t i, uint64_t a, uint64_t ra) const {
    bool ok = true;
    if (i < c.n) {
      (void)entry_len(c, i, &ok);
      c.sums[i] = ra;
    }
    ix::wave_count_to(ctl + mvk::WW_CTL_BAD, !ok);
  }
};

struct Sums {
  const uint64_t* s;
  uint64_t n, total;
  __device__ uint64_t operator()(uint64_t i) const { return i < n ? s[i] : total; }
};

// The first i in [lo, n) with S(i + 1) > T, or n, on the whole wave (the result is wave-uniform).
// S is strictly increasing. Invariant: S(i + 1) <= T below lo; hi == n or S(hi + 1) > T.
struct FirstAbove {
  Sums S;
  __device__ uint64_t operator()(uint64_t lo, uint64_t T) const {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t hi = S.n;
    if (hi - lo > 64) {  // the mean entry length's guess: 64 entries around it
      const double est = (double)(T - S(lo)) * (double)S.n / (double)S.total;
      const uint64_t e = est < (double)(hi - lo) ? lo + (uint64_t)est : hi;
      uint64_t w0 = e > lo + 32 ? e - 32 : lo;
      if (w0 > hi - 64) w0 = hi - 64;
      const u64 m = __ballot(S(w0 + lane + 1) > T);
      if (m == 0) {
        lo = w0 + 64;
      } else {
        const uint32_t f = (uint32_t)__ffsll((long long)m) - 1;
        if (f) return w0 + f;
        hi = w0;
      }
    }
    while (lo < hi) {  // 64 probes a round, evenly over [lo, hi)
      const uint64_t span = hi - lo, step = (span + 63) / 64;
      const uint64_t idx = lo + lane * step;
      const u64 m = __ballot(idx < hi && S(idx + 1) > T);
      if (m == 0) {
        lo += (span - 1) / step * step + 1;
      } else {
        const uint32_t f = (uint32_t)__ffsll((long long)m) - 1;
        hi = lo + f * step;
        if (f) lo += (f - 1) * step + 1;
      }
    }
    return lo;
  }
};

__global__ void __launch_bounds__(64) k_ww_cross(const WalWriteCall c, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x;
  if (ctl[mvk::WW_CTL_BAD]) {
    if (lane == 0) ctl[mvk::WW_CTL_NC] = 0, ctl[mvk::WW_CTL_END] = c.start;
    return;
  }
  const Sums S{c.sums, c.n, ctl[mvk::WW_CTL_TOTAL]};
  const FirstAbove find{S};
  uint64_t cur = 0, g = 0, gap = 0, nc = 0;
  while (wl::cross_step(c.n, c.start, c.map_bits, S, find, &cur, &g, &gap)) {
    if (!gap) continue;
    if (lane == 0 && nc < c.n) c.cross_first[nc] = cur, c.cross_shift[nc] = g;  // (one gap per entry at most)
    nc++;
  }
  if (lane == 0) ctl[mvk::WW_CTL_NC] = nc < c.n ? nc : c.n, ctl[mvk::WW_CTL_END] = c.start + g + S.total;
}

__global__ void __launch_bounds__(ix::WG) k_ww_pos(const WalWriteCall c, const u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * ix::WG + threadIdx.x;
  if (i >= c.n || ctl[mvk::WW_CTL_BAD]) return;
  c.pos[i] = c.start + wl::shift_at(c.cross_first, c.cross_shift, ctl[mvk::WW_CTL_NC], i) + c.sums[i];
}

// ------------------------------------------------------------------ the bytes
// zero bytes out[lo, hi) on the whole wave: aligned 8-byte words, the edges byte by byte
MV_DEV void zero_fill(uint8_t* __restrict__ out, uint64_t lo, uint64_t hi) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t a = (lo + 7) & ~7ull, b = hi & ~7ull;
  if (a >= b) {
    for (uint64_t p = lo + lane; p < hi; p += 64) out[p] = 0;
    return;
  }
  if (lo + lane < a) out[lo + lane] = 0;
  for (uint64_t p = a + 8 * (uint64_t)lane; p < b; p += 512) *reinterpret_cast<uint64_t*>(out + p) = 0;
  if (b + lane < hi) out[b + lane] = 0;
}

// the fold's words to the body: dst + q is 4-byte aligned for every q of the grid
struct BodySink {
  uint8_t* dst;
  MV_DEV void operator()(int64_t q, uint32_t w) const {
    if (q >= 0) {
      *reinterpret_cast<uint32_t*>(dst + q) = w;
    } else {
      for (int k = (int)-q; k < 4; k++) dst[q + k] = (uint8_t)(w >> (8 * k));
    }
  }
};

__global__ void __launch_bounds__(WG) MV_WW_ATTR k_ww_emit(const WalWriteCall c, const uint32_t* __restrict__ tables,
                                                u64* __restrict__ ctl) {
  __shared__ Lds L;
  lds_fill(L, tables);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (WG / 64);
  const uint32_t* tbyte = tables + A_WORDS + S_WORDS;
  const uint32_t* S = s_tab(L, tables);
  for (uint64_t e = blockIdx.x * (WG / 64) + threadIdx.x / 64; e < c.n; e += waves) {
    const uint64_t* row = c.entries + wl::ENTRY_WORDS * e;
    const uint64_t tag = bcast64(row[0]), off = bcast64(row[1]), len = bcast64(row[2]), next = bcast64(row[3]);
    uint64_t prev_end = 0;
    if (e) {
      const uint64_t* pr = row - wl::ENTRY_WORDS;
      prev_end = bcast64(c.pos[e - 1]) - c.start + wl::HEADER + wl::body_len(bcast64(pr[0]), bcast64(pr[2]));
    }
    const wl::Span sp = wl::span_of(prev_end, bcast64(c.pos[e]) - c.start, tag, len);
    // (the host has refused what does not fit: these hold, and nothing is touched where one does not)
    if (sp.gap0 > sp.at || sp.end < sp.at || sp.end > c.cap || len > c.buf_bytes || off > c.buf_bytes - len) {
      if (lane == 0) atomicOr(ctl + mvk::WW_CTL_ERR, 1ull);
      continue;
    }
    zero_fill(c.out, sp.gap0, sp.at);
    const bool own = (uint32_t)tag == wl::TAG_OWN;
    const uint64_t tail = len < (sp.end & 3) ? len : (sp.end & 3);
    const uint64_t a = off, bE = off + len - tail;
    uint32_t raw = crc_raw_wave(c.buf, a, bE, L, S, BodySink{c.out + sp.body});
    if (own) {
      uint32_t s0 = 0xffffffffu;
      for (int k = 0; k < 8; k++) s0 = (s0 >> 8) ^ tbyte[(s0 ^ (uint32_t)(next >> (8 * k))) & 255];
      raw ^= zeros_shift(L, S, tbyte, ~s0, bE - a);
    }
    for (uint64_t k = 0; k < tail; k++) {
      const uint32_t byte = c.buf[bE + k];
      raw = (raw >> 8) ^ tbyte[(raw ^ byte) & 255];
      if (lane == k) c.out[sp.end - tail + k] = (uint8_t)byte;
    }
    uint64_t hw[2];
    wl::header_words(~raw, tag, len, hw);
    if (lane < 16) c.out[sp.at + lane] = (uint8_t)(hw[lane >> 3] >> (8 * (lane & 7)));
    else if (own && lane < 24) c.out[sp.at + lane] = (uint8_t)(next >> (8 * (lane - 16)));
  }
}

}  // namespace ww
}  // namespace mv

namespace mvk {

hipError_t launch_wal_write_layout(const WalWriteCall& c, void* wg, uint64_t* ctl, hipStream_t s) {
  if (c.n == 0) return hipSuccess;
  using namespace mv::ww;
  mv::ix::compact_pass(LenScan{c, (u64*)ctl}, c.n, wg_scan_of(wg, c.n), ctl + WW_CTL_TOTAL, nullptr, nullptr, s);
  hipLaunchKernelGGL(k_ww_cross, dim3(1), dim3(64), 0, s, c, (u64*)ctl);
  hipLaunchKernelGGL(k_ww_pos, dim3(mv::ix::grid_of(c.n)), dim3(mv::ix::WG), 0, s, c, (const u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_wal_write_emit(const WalWriteCall& c, const uint32_t* tables, uint64_t* ctl, int cus, hipStream_t s) {
  if (c.n == 0) return hipSuccess;
  // a persistent grid of the workgroups that are resident at once: the kernel's registers, not the
  // LDS, bound them (crc_grid's two per CU would refill the tables and split the entries unevenly)
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mv::ww::k_ww_emit, mv::wal::WG, 0);
  if (e != hipSuccess) return e;
  const uint64_t per_wg = mv::wal::WG / 64, want = (c.n + per_wg - 1) / per_wg;
  const uint64_t cap = (uint64_t)(per_cu < 1 ? 1 : per_cu) * (uint64_t)(cus < 1 ? 1 : cus);
  hipLaunchKernelGGL(mv::ww::k_ww_emit, dim3((uint32_t)(want < cap ? want : cap)), dim3(mv::wal::WG), 0, s, c, tables,
                     (mv::ww::u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
