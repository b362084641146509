// The suspended-block store and the connect sweep.
// mv_connect_blocks: the suspend / unlock cascade of add_blocks (block_manager.rs:102-131) as a
// least fixed point -- a suspended block is stored exactly when all its includes are stored. A
// record holds slots of the table, not keys: a level's check is one 8-byte load per include, and
// the reference words of a row are read from the block's own slot. Level l is four launches on
// one stream:
//   k_pb_check   a wave per record not connected yet: every include's state is STORED (and its
//                own is not). It reads only states raised by earlier launches.
//   LevelRows    (index_dev.h's compaction pass: count, k_ix_scan, list) the hits per workgroup
//                and their places behind the rows so far; a hit writes its row (below the cap),
//                notes its level and raises its own state by atomicMax. Nothing in the list launch
//                reads a state.
// Within a level the scan orders rows by record, which is arrival order: compaction is stable
// and appends go in block order. No lane waits for another; the host enqueues levels until one
// lists nothing, at most records + 1 of them.
// The memory model is index_dev.h's.
#include "index_dev.h"

namespace mv::ix {

__global__ void __launch_bounds__(WG) k_pb_own_slots(const u64* __restrict__ item, uint64_t ncand,
                                                     uint64_t* __restrict__ cand_slot) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (r < ncand) cand_slot[r] = item[r] & SLOT_MASK;
}

// the NEW blocks among the candidates join the store in block order; weights: the block, its includes
struct AppendNew {
  static constexpr int WEIGHTS = 2;
  AcceptArrays a;
  uint64_t ncand;
  const uint64_t* cand_slot;
  PendStore p;
  uint64_t nb0, ni0;
  uint64_t* cand_dst;
  __device__ void weigh(uint64_t r, uint64_t* nw, uint64_t* k) const {
    *nw = r < ncand && a.state[a.cand_blk[r]] == MV_ACC_NEW;
    *k = *nw ? a.kc[a.cand_blk[r]] : 0;
  }
  __device__ void place(uint64_t r, uint64_t nw, uint64_t rb, uint64_t k, uint64_t ib) const {
    if (r >= ncand) return;
    rb += nb0, ib += ni0;
    cand_dst[r] = nw ? ib : mvk::IX_NO_SRC;
    if (!nw) return;
    p.slot[rb] = cand_slot[r];
    p.ibase[rb] = ib;
    p.blk[rb] = a.cand_blk[r];
    p.kc[rb] = (uint32_t)k;
  }
};
// one lane per include of the candidates (k_acc_inc_src's shape): its slot into its block's record
__global__ void __launch_bounds__(WG) k_pb_app_inc(AcceptArrays a, uint64_t ncand, uint64_t ninc, const u64* __restrict__ item,
                                                   const uint64_t* __restrict__ cand_dst, PendStore p) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= ninc) return;
  const uint64_t lo = cand_of_include(a.inc_base, ncand, j);
  const uint64_t q = j - a.inc_base[lo];
  if (cand_dst[lo] != mvk::IX_NO_SRC && q < a.kc[a.cand_blk[lo]]) p.inc[cand_dst[lo] + q] = item[j] & SLOT_MASK;
}

__global__ void __launch_bounds__(WG) k_pb_check(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                 const uint32_t* __restrict__ lvl, uint8_t* __restrict__ hit) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // the same for the whole wave
  const uint32_t lane = threadIdx.x & 63;
  if (b >= nb) return;
  bool ok = lvl[b] == 0 && slot_state(slots, p.slot[b]) != MV_REF_STORED;
  if (ok) {
    const uint64_t base = p.ibase[b];
    const uint32_t kc = p.kc[b];
    for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave leaves together
      const uint32_t q = q0 + lane;
      const bool bad = q < kc && slot_state(slots, p.inc[base + q]) != MV_REF_STORED;
      if (__ballot(bad)) {
        ok = false;
        break;
      }
    }
  }
  if (lane == 0) hit[b] = ok;
}
// the hits of a level, in record order, behind the rows so far
struct LevelRows {
  static constexpr int WEIGHTS = 1;
  u64* slots;
  PendStore p;
  uint64_t nb;
  const uint8_t* hit;
  uint32_t* lvl;
  uint64_t level;
  uint64_t* out;
  uint64_t cap;
  u64* ctl;
  uint32_t* row_of;
  __device__ void weigh(uint64_t b, uint64_t* h) const { *h = b < nb && hit[b]; }
  __device__ void place(uint64_t b, uint64_t h, uint64_t r) const {
    if (h) {
      u64* slot = slots + SLOT_WORDS * p.slot[b];
      lvl[b] = (uint32_t)level + 1;
      if (row_of) row_of[b] = (uint32_t)r;  // (with a DAG store: its record order is the row order)
      if (r < cap) {
        const uint64_t blk = p.blk[b];
        copy_key(out + 8 * r, slot);  // (the key: written by an earlier launch)
        out[8 * r + 6] = blk;
        out[8 * r + 7] = level;
      }
      atomicMax(meta_of(slot), (uint32_t)MV_REF_STORED);
    }
    wave_count_to(ctl + mvk::IX_CTL_STORED, h);
  }
};

// compaction: the records whose own reference is not STORED stay, in order; weights: the record, its includes
struct KeepPending {
  static constexpr int WEIGHTS = 2;
  const u64* slots;
  PendStore p, q;
  uint64_t nb;
  uint64_t* newbase;
  uint8_t* state;
  uint64_t n_state;
  __device__ void weigh(uint64_t b, uint64_t* keep, uint64_t* k) const {
    *keep = b < nb && slot_state(slots, p.slot[b]) != MV_REF_STORED;
    *k = *keep ? p.kc[b] : 0;
  }
  __device__ void place(uint64_t b, uint64_t keep, uint64_t rb, uint64_t k, uint64_t ib) const {
    if (b >= nb) return;
    newbase[b] = keep ? ib : mvk::IX_NO_SRC;
    if (!keep) return;
    q.slot[rb] = p.slot[b];
    q.ibase[rb] = ib;
    q.blk[rb] = mvk::IX_NO_SRC;  // the next call finds it suspended by an earlier one
    q.kc[rb] = (uint32_t)k;
    if (p.blk[b] < n_state) state[p.blk[b]] = MV_ACC_SUSPENDED;  // (n_state is 0 without a state array)
  }
};
__global__ void __launch_bounds__(WG) k_pb_keep_inc(PendStore p, PendStore q, uint64_t nb, const uint64_t* __restrict__ newbase) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (b >= nb || newbase[b] == mvk::IX_NO_SRC) return;
  const uint64_t from = p.ibase[b], to = newbase[b];
  const uint32_t kc = p.kc[b];
  for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) q.inc[to + i] = p.inc[from + i];
}

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_pend_own_slots(const uint64_t* item, uint64_t ncand, uint64_t* cand_slot, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_own_slots, dim3(grid_of(ncand)), dim3(WG), 0, s, (const u64*)item, ncand, cand_slot);
  return hipGetLastError();
}

hipError_t launch_pend_append(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, const uint64_t* item,
                              const uint64_t* cand_slot, uint64_t* cand_dst, const PendStore& p, uint64_t nb0, uint64_t ni0,
                              uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  compact_pass(AppendNew{a, ncand, cand_slot, p, nb0, ni0, cand_dst}, ncand, wg_scan_of(wg, ncand), ctl + IX_CTL_PB_NB,
               ctl + IX_CTL_PB_NI, nullptr, s);
  if (ninc) hipLaunchKernelGGL(k_pb_app_inc, dim3(grid_of(ninc)), dim3(WG), 0, s, a, ncand, ninc, (const u64*)item, cand_dst, p);
  return hipGetLastError();
}

hipError_t launch_pend_level(const IndexTable& t, const PendStore& p, uint64_t nb, uint32_t* lvl, uint8_t* hit,
                             uint64_t level, uint64_t* wg, uint64_t* out, uint64_t cap, uint64_t* ctl, int lv_word,
                             uint32_t* row_of, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_check, dim3(grid_of(64 * nb)), dim3(WG), 0, s, (const u64*)t.slots, p, nb, lvl, hit);
  compact_pass(LevelRows{(u64*)t.slots, p, nb, hit, lvl, level, out, cap, (u64*)ctl, row_of}, nb, wg_scan_of(wg, nb),
               ctl + lv_word, nullptr, ctl + IX_CTL_PB_ROWS, s);
  return hipGetLastError();
}

hipError_t launch_pend_compact(const IndexTable& t, const PendStore& p, const PendStore& q, uint64_t nb, uint64_t* newbase,
                               uint8_t* state, uint64_t n_state, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  compact_pass(KeepPending{(const u64*)t.slots, p, q, nb, newbase, state, state ? n_state : 0}, nb, wg_scan_of(wg, nb),
               ctl + IX_CTL_PB_NB, ctl + IX_CTL_PB_NI, nullptr, s);
  hipLaunchKernelGGL(k_pb_keep_inc, dim3(grid_of(64 * nb)), dim3(WG), 0, s, p, q, nb, newbase);
  return hipGetLastError();
}

}  // namespace mvk
