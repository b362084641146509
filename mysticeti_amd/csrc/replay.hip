// mv_wal_replay on the device: what BlockStore::open's replay loop (block_store.rs:66-103) does
// with the entries the WAL walk and crc pass (wal.hip) list, up to the block-store index. The
// entry rules are those of wal_entry.h; the blocks found are verified in place in the image by
// the block pipeline (engine_blocks.cpp enqueue_blocks) between k_replay_list and k_replay_rows.
//
//   k_replay_select   one lane per entry: unknown tags and tag-3 payloads without a header become
//                     the entry's status; counts the entries that carry a block per workgroup
//   (k_ix_scan)       index.hip's scan of the per-workgroup counts, the block total
//   k_replay_list     one lane per entry: the block's (offset, length, entry) at its scanned
//                     position (index_dev.h's workgroup prefix), so the list is in iteration order
//   k_replay_rows     one lane per listed block: the row from the block's first 56 bytes; a block
//                     that does not parse, then an authority outside the committee, become the
//                     entry's status (decode before authority, block_store.rs:73-74, 424-428)
//   k_replay_cut      one lane per entry: the first entry whose status is not OK (minimum)
//   k_replay_summary  one lane per row and per entry: the rows kept, last_seen_by_authority (LDS
//                     per workgroup, then global atomicMax), highest_round, the last own block
//                     and the last state entry
//   k_replay_finish   one lane: the summary words and the two counts
//
// Every image byte is untrusted. A row is read only from a block the pipeline parsed, whose
// listed length (checked again here) covers the 56 bytes; the own-block header lies inside the
// payload by wal_entry.h's rule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_dev.h"
#include "wal_entry.h"

namespace mv {
namespace rp {

constexpr int WG = ix::WG;  // (the per-workgroup counts go through the index's scan)

__device__ inline uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
constexpr int MAX_AUTH = 512;  // mv_set_committee's limit

__device__ inline bool carries_block(const uint64_t* pos, const uint32_t* tag, const uint32_t* len, const uint8_t* st,
                                     uint64_t e, uint64_t size, we::Entry& c) {
  if (st[e] != MV_WAL_OK) return false;
  c = we::classify(tag[e], pos[e], len[e], size);
  return c.block;
}

__global__ void __launch_bounds__(WG) k_replay_select(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ tag,
                                                      const uint32_t* __restrict__ len, uint8_t* __restrict__ st,
                                                      uint64_t n, uint64_t size, uint64_t* __restrict__ wgcount) {
  const uint64_t e = (uint64_t)blockIdx.x * WG + threadIdx.x;
  int blk = 0;
  if (e < n && st[e] == MV_WAL_OK) {
    const we::Entry c = we::classify(tag[e], pos[e], len[e], size);
    if (c.status != MV_WAL_OK) st[e] = (uint8_t)c.status;
    blk = c.block;
  }
  const int cnt = __syncthreads_count(blk);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = (uint64_t)cnt;
}

// cap: the lists' length (the host sizes them by the entry count)
__global__ void __launch_bounds__(WG) k_replay_list(const uint64_t* __restrict__ pos, const uint32_t* __restrict__ tag,
                                                    const uint32_t* __restrict__ len, const uint8_t* __restrict__ st,
                                                    uint64_t n, uint64_t size, const uint64_t* __restrict__ wgbase,
                                                    uint64_t* __restrict__ blk_off, uint64_t* __restrict__ blk_len,
                                                    uint64_t* __restrict__ blk_ent, uint64_t cap) {
  const uint64_t e = (uint64_t)blockIdx.x * WG + threadIdx.x;
  we::Entry c{};
  const bool blk = e < n && carries_block(pos, tag, len, st, e, size, c);
  uint64_t tot;
  const uint64_t r = wgbase[blockIdx.x] + ix::wg_excl(blk, &tot);
  if (!blk || r >= cap) return;
  blk_off[r] = c.off;
  blk_len[r] = c.len;
  blk_ent[r] = e;
}

__global__ void __launch_bounds__(WG) k_replay_rows(const uint8_t* __restrict__ img, const uint64_t* __restrict__ blk_off,
                                                    const uint64_t* __restrict__ blk_len,
                                                    const uint64_t* __restrict__ blk_ent,
                                                    const uint8_t* __restrict__ blk_status, uint64_t nb,
                                                    const uint32_t* __restrict__ tag, uint8_t* __restrict__ st,
                                                    uint64_t n, uint32_t n_auth, uint64_t* __restrict__ rows) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (r >= nb) return;
  const uint64_t e = blk_ent[r], off = blk_off[r];
  if (e >= n) return;
  if (blk_status[r] == MV_BLOCK_PARSE_ERROR || blk_len[r] < we::REF_BYTES) {
    st[e] = MV_WAL_BLOCK_DECODE;
    return;
  }
  const uint64_t authority = ld64(img + off);
  if (authority >= n_auth) {
    st[e] = MV_WAL_UNKNOWN_AUTHORITY;
    return;
  }
  uint64_t* row = rows + we::ROW_WORDS * r;
  row[0] = e;
  row[1] = off;
  row[2] = blk_len[r];
  row[3] = authority;
  row[4] = ld64(img + off + 8);
  for (int k = 0; k < 4; k++) row[5 + k] = ld64(img + off + 24 + 8 * k);
  row[9] = tag[e] == we::TAG_OWN_BLOCK ? ld64(img + off - we::OWN_HEADER) : we::NONE;
}

// *ff = the least entry index whose status is not OK (preset to NONE). Entry indices ascend with
// the lane, so the first failing lane of a wave holds the wave's minimum: one atomic per wave.
__global__ void __launch_bounds__(WG) k_replay_cut(const uint8_t* __restrict__ st, uint64_t n,
                                                   unsigned long long* __restrict__ ff) {
  const uint64_t e = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool bad = e < n && st[e] != MV_WAL_OK;
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicMin(ff, (unsigned long long)e);
}

// acc: [0] highest round, [1] last own row + 1, [2] last state entry + 1 (all preset to 0);
// *nrows (preset to 0) = rows of entries before *ff; last_seen preset to 0
__global__ void __launch_bounds__(WG) k_replay_summary(const uint64_t* __restrict__ rows,
                                                       const uint64_t* __restrict__ blk_ent, uint64_t nb,
                                                       const uint32_t* __restrict__ tag, uint64_t n,
                                                       const unsigned long long* __restrict__ ff, uint32_t n_auth,
                                                       unsigned long long* __restrict__ acc,
                                                       unsigned long long* __restrict__ nrows,
                                                       unsigned long long* __restrict__ last_seen) {
  __shared__ unsigned long long seen[MAX_AUTH];
  __shared__ unsigned long long top[3];
  for (uint32_t a = threadIdx.x; a < MAX_AUTH; a += WG) seen[a] = 0;
  if (threadIdx.x < 3) top[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t first_bad = *ff;
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i < nb) {
    const uint64_t e = blk_ent[i];
    if (e < first_bad) {  // a kept row: its entry is OK, so k_replay_rows wrote it (authority < n_auth)
      const uint64_t* row = rows + we::ROW_WORDS * i;
      const uint64_t a = row[3], rnd = row[4];
      if (a < n_auth && a < MAX_AUTH && rnd) atomicMax(&seen[a], (unsigned long long)rnd);
      if (rnd) atomicMax(&top[0], (unsigned long long)rnd);
      if (e < n && tag[e] == we::TAG_OWN_BLOCK) atomicMax(&top[1], (unsigned long long)(i + 1));
      if (i + 1 == nb || blk_ent[i + 1] >= first_bad) *nrows = i + 1;  // (one lane: entries ascend)
    }
  }
  if (i < n && i < first_bad && tag[i] == we::TAG_STATE) atomicMax(&top[2], (unsigned long long)(i + 1));
  __syncthreads();
  for (uint32_t a = threadIdx.x; a < n_auth && a < MAX_AUTH; a += WG)
    if (seen[a]) atomicMax(&last_seen[a], seen[a]);
  if (threadIdx.x < 3 && top[threadIdx.x]) atomicMax(&acc[threadIdx.x], top[threadIdx.x]);
}

// summary[1], [2]: 0 - 1 = UINT64_MAX where there is none; counts = {entries, rows}
__global__ void k_replay_finish(const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ ff,
                                const unsigned long long* __restrict__ nrows, uint64_t n, uint64_t* __restrict__ summary,
                                uint64_t* __restrict__ counts) {
  if (threadIdx.x || blockIdx.x) return;
  summary[0] = acc[0];
  summary[1] = acc[1] - 1;
  summary[2] = acc[2] - 1;
  counts[0] = *ff < n ? *ff + 1 : n;
  counts[1] = *nrows;
}

static inline uint32_t grid_of(uint64_t items) { return (uint32_t)((items + WG - 1) / WG); }

}  // namespace rp
}  // namespace mv

namespace mvk {

uint64_t replay_groups(uint64_t n) { return (n + mv::rp::WG - 1) / mv::rp::WG; }

hipError_t launch_replay_select(const ReplayEntries& en, uint64_t size, uint64_t* wgcount, uint64_t* wgbase,
                                uint64_t* nb, hipStream_t s) {
  if (en.n == 0) return hipSuccess;
  const uint64_t nwg = replay_groups(en.n);
  hipLaunchKernelGGL(mv::rp::k_replay_select, dim3((uint32_t)nwg), dim3(mv::rp::WG), 0, s, en.pos, en.tag, en.len,
                     en.status, en.n, size, wgcount);
  (void)launch_index_scan(wgcount, nwg, wgbase, nb, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_replay_list(const ReplayEntries& en, uint64_t size, const uint64_t* wgbase, const ReplayBlocks& bl,
                              hipStream_t s) {
  if (en.n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::rp::k_replay_list, dim3((uint32_t)replay_groups(en.n)), dim3(mv::rp::WG), 0, s, en.pos, en.tag,
                     en.len, en.status, en.n, size, wgbase, bl.off, bl.len, bl.ent, bl.cap);
  return hipGetLastError();
}

hipError_t launch_replay_rows(const uint8_t* img, const ReplayEntries& en, const ReplayBlocks& bl, uint32_t n_auth,
                              uint64_t* rows, hipStream_t s) {
  if (bl.n == 0) return hipSuccess;
  hipLaunchKernelGGL(mv::rp::k_replay_rows, dim3(mv::rp::grid_of(bl.n)), dim3(mv::rp::WG), 0, s, img, bl.off, bl.len,
                     bl.ent, bl.status, bl.n, en.tag, en.status, en.n, n_auth, rows);
  return hipGetLastError();
}

hipError_t launch_replay_summary(const ReplayEntries& en, const ReplayBlocks& bl, const uint64_t* rows, uint32_t n_auth,
                                 uint64_t* ctl, uint64_t* summary, uint64_t* last_seen, uint64_t* counts,
                                 hipStream_t s) {
  unsigned long long* c = (unsigned long long*)ctl;
  if (en.n) {
    hipLaunchKernelGGL(mv::rp::k_replay_cut, dim3(mv::rp::grid_of(en.n)), dim3(mv::rp::WG), 0, s, en.status, en.n,
                       c + REPLAY_CTL_FF);
    const uint64_t items = en.n > bl.n ? en.n : bl.n;
    hipLaunchKernelGGL(mv::rp::k_replay_summary, dim3(mv::rp::grid_of(items)), dim3(mv::rp::WG), 0, s, rows, bl.ent,
                       bl.n, en.tag, en.n, c + REPLAY_CTL_FF, n_auth, c + REPLAY_CTL_ACC, c + REPLAY_CTL_NROWS,
                       (unsigned long long*)last_seen);
  }
  hipLaunchKernelGGL(mv::rp::k_replay_finish, dim3(1), dim3(64), 0, s, c + REPLAY_CTL_ACC, c + REPLAY_CTL_FF,
                     c + REPLAY_CTL_NROWS, en.n, summary, counts);
  return hipGetLastError();
}

}  // namespace mvk
