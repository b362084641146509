// mv_encode_blocks on the device: the bincode of the blocks Core::try_new_block makes (core.rs:264-291,
// types.rs:93-114, 155-218, data.rs:43-52) from head words, include rows and payload strings. The
// rules -- payload check, head checks, length, piece table -- are encode_walk.h's; this file is the
// three kernels that run them and the scans between them.
//
//   k_en_check   a lane per payload: its span, the statement walk, the end on the last byte; the
//                statement count and the body length. A payload listed by several blocks is checked
//                once. Then the exclusive scan of the body lengths over the whole payload list
//                (k_ix_scan through compact_pass): a block's payloads are a run of that list, so its
//                piece boundaries are differences of the scan's entries.
//   k_en_size    a lane per block: the head checks, the sum over its payloads, status, length and
//                statement count. Then the scan of the padded lengths: out_off in block order, no
//                atomics. The same pass lists the blocks of at least EN_WG_BYTES. The total comes
//                back to the host, with the length of that list beside it in the same copy.
//   k_en_write   a wave per block below EN_WG_BYTES, a workgroup per block of the list. The
//                block's boundaries S_0 .. S_np go to LDS, a step of one entry per lane at a time,
//                when there are at most EN_TILE payloads (a block of more reads them from the scan's
//                array). Lanes stride over the destination words of the padded span; each assembles
//                its word from the pieces it straddles (BlockSrc::dest_word: binary search in the
//                boundaries, peek8 reads of the payload at whatever alignment it has) and writes it
//                with one aligned 8-byte store. No byte stores, no read-modify-write: a block starts
//                on an 8-byte boundary and its padding is its own, so no word is shared.
//
// Memory safety: k_en_size holds every run against m and p before an index is formed; k_en_write
// checks the head again, the block's span against cap, and through BlockSrc every source index and
// offset where it becomes an address. A failed check adds to ctl[EN_CTL_ERR] (the host returns
// MV_E_HIP) and the access is skipped. Nothing is written outside [out_off, out_off + padded length).
#include "index_dev.h"

#include "encode_walk.h"

namespace mv::ix {

using mvk::EncodeCall;
using namespace mv::en;

namespace {

__device__ inline void en_err(u64* ctl) { atomicAdd(ctl + mvk::EN_CTL_ERR, 1ull); }

__global__ void __launch_bounds__(WG) k_en_check(EncodeCall c) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= c.p) return;
  uint64_t count, body;
  const bool ok = check_payload(c.payload_buf, c.payload_bytes, c.payload_off[j], c.payload_len[j], &count, &body);
  c.pay_ok[j] = ok;
  c.pay_count[j] = count;
  c.pay_body[j] = body;
}

// pre[j] = the bodies of the payloads before j, pre[p] = all of them
struct BodyScan {
  static constexpr int WEIGHTS = 1;
  EncodeCall c;
  __device__ void weigh(uint64_t j, uint64_t* w) const { *w = j < c.p ? c.pay_body[j] : 0; }
  __device__ void place(uint64_t j, uint64_t w, uint64_t ex) const {
    if (j >= c.p) return;
    c.pre[j] = ex;
    if (j + 1 == c.p) c.pre[c.p] = ex + w;
  }
};

__global__ void __launch_bounds__(WG) k_en_size(EncodeCall c) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= c.n) return;
  uint64_t len, count;
  const uint32_t st = size_block(c.heads + HEAD_WORDS * i, c.m, c.p, c.pay_ok, c.pay_body, c.pay_count, &len, &count);
  c.status[i] = (uint8_t)st;
  c.out_len[i] = len;
  c.blk_count[i] = count;
}

// out_off[i] = the padded lengths of the blocks before i; big[] = the blocks a workgroup writes, in order
struct SpanScan {
  static constexpr int WEIGHTS = 2;
  EncodeCall c;
  __device__ void weigh(uint64_t i, uint64_t* w, uint64_t* big) const {
    const uint64_t len = i < c.n ? c.out_len[i] : 0;
    *w = round_up8(len);
    *big = len >= mvk::EN_WG_BYTES;
  }
  __device__ void place(uint64_t i, uint64_t, uint64_t ex, uint64_t big, uint64_t rank) const {
    if (i >= c.n) return;
    c.out_off[i] = ex;
    if (big && rank < c.n) c.big[rank] = (uint32_t)i;
  }
};

struct ErrCount {
  u64* ctl;
  __device__ void operator()() const { en_err(ctl); }
};
// S_j of the block whose payloads start at pay0: from LDS, or from the scan's array
struct Boundaries {
  const uint64_t* tile;  // null: no tile
  const uint64_t* pre;
  uint64_t pay0;
  __device__ uint64_t operator()(uint64_t j) const { return tile ? tile[j] : pre[pay0 + j] - pre[pay0]; }
};

// WHOLE_WG: workgroup g writes block big[g] (nbig of them); else wave w of the grid writes block w
template <bool WHOLE_WG>
__global__ void __launch_bounds__(WG) k_en_write(EncodeCall c, uint32_t nbig, u64* __restrict__ ctl) {
  constexpr uint32_t TEAMS = WHOLE_WG ? 1 : WG / 64, WIDTH = WHOLE_WG ? WG : 64;
  __shared__ uint64_t tiles[TEAMS][mvk::EN_TILE + 1];
  const uint32_t team = WHOLE_WG ? 0 : threadIdx.x / 64, lane = WHOLE_WG ? threadIdx.x : threadIdx.x & 63;
  // (every condition up to the barrier is the same for all lanes of the team)
  if (WHOLE_WG && blockIdx.x >= nbig) return;
  const uint64_t i = WHOLE_WG ? c.big[blockIdx.x] : (uint64_t)blockIdx.x * TEAMS + team;
  if (i >= c.n || c.status[i] != MV_ENCODE_OK) return;
  const uint64_t len = c.out_len[i], off = c.out_off[i], padded = round_up8(len);
  if ((len >= mvk::EN_WG_BYTES) != WHOLE_WG) return;
  const Inputs in{c.heads, c.includes, c.m, c.payload_buf, c.payload_bytes, c.payload_off, c.payload_len, c.p};
  Shape sh;
  if (!span_ok(off, len, c.cap) || !shape_of(in, i, c.pre, c.blk_count[i], len, &sh)) {
    if (lane == 0) en_err(ctl);
    return;
  }
  const bool tiled = sh.np <= mvk::EN_TILE;
  uint64_t* tile = tiles[team];
  if (tiled) {
    const uint64_t base = c.pre[sh.pay0];
    for (uint64_t j = lane; j <= sh.np; j += WIDTH) tile[j] = c.pre[sh.pay0 + j] - base;
    if (WHOLE_WG) __syncthreads();
    else wave_sync();
  }
  const BlockSrc<Boundaries, ErrCount> src{in, i, sh, Boundaries{tiled ? tile : nullptr, c.pre, sh.pay0}, ErrCount{ctl}};
  uint64_t* dst = reinterpret_cast<uint64_t*>(c.out + off);  // (8-byte aligned: out is, off checked above)
  for (uint64_t w = lane; w < padded / 8; w += WIDTH) dst[w] = src.dest_word(8 * w);
}

}  // namespace
}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_encode_check(const EncodeCall& c, void* wg, uint64_t* ctl, hipStream_t s) {
  if (c.p == 0) return hipMemsetAsync(c.pre, 0, 8, s);
  hipLaunchKernelGGL(k_en_check, dim3(grid_of(c.p)), dim3(WG), 0, s, c);
  compact_pass(BodyScan{c}, c.p, wg_scan_of(wg, c.p), ctl + EN_CTL_BODY, nullptr, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_encode_size(const EncodeCall& c, void* wg, uint64_t* ctl, hipStream_t s) {
  if (c.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_en_size, dim3(grid_of(c.n)), dim3(WG), 0, s, c);
  compact_pass(SpanScan{c}, c.n, wg_scan_of(wg, c.n), ctl + EN_CTL_TOTAL, ctl + EN_CTL_NBIG, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_encode_write(const EncodeCall& c, uint64_t nbig, uint64_t* ctl, hipStream_t s) {
  if (c.n == 0) return hipSuccess;
  if (nbig > c.n) return hipErrorInvalidValue;
  if (nbig < c.n)
    hipLaunchKernelGGL(k_en_write<false>, dim3((c.n + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, s, c, 0u, (u64*)ctl);
  if (nbig) hipLaunchKernelGGL(k_en_write<true>, dim3((uint32_t)nbig), dim3(WG), 0, s, c, (uint32_t)nbig, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
