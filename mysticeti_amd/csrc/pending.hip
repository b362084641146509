// The suspended-block store and the connect sweep.
// mv_connect_blocks: the suspend / unlock cascade of add_blocks (block_manager.rs:102-131) as a
// least fixed point -- a suspended block is stored exactly when all its includes are stored. A
// record holds slots of the table, not keys: a level's check is one 8-byte load per include, and
// the reference words of a row are read from the block's own slot. Level l is four launches on
// one stream:
//   k_pb_check   a wave per record not connected yet: every include's state is STORED (and its
//                own is not). It reads only states raised by earlier launches.
//   k_pb_count, k_ix_scan   the hits per workgroup and their places behind the rows so far
//   k_pb_list    a hit writes its row (below the cap), notes its level and raises its own state
//                by atomicMax. Nothing in this launch reads a state.
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

// the NEW blocks among the candidates and their includes, per workgroup
__device__ inline bool app_new(const AcceptArrays& a, uint64_t ncand, uint64_t r, uint64_t* k) {
  const bool nw = r < ncand && a.state[a.cand_blk[r]] == MV_ACC_NEW;
  *k = nw ? a.kc[a.cand_blk[r]] : 0;
  return nw;
}
__global__ void __launch_bounds__(WG) k_pb_app_count(AcceptArrays a, uint64_t ncand, uint64_t* __restrict__ wg_a,
                                                     uint64_t* __restrict__ wg_b) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t k;
  const bool nw = app_new(a, ncand, r, &k);
  uint64_t tb, tk;
  (void)wg_excl(nw, &tb);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}
__global__ void __launch_bounds__(WG) k_pb_app_list(AcceptArrays a, uint64_t ncand, const uint64_t* __restrict__ cand_slot,
                                                    const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b,
                                                    PendStore p, uint64_t nb0, uint64_t ni0, uint64_t* __restrict__ cand_dst) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t k;
  const bool nw = app_new(a, ncand, r, &k);
  uint64_t tb, tk;
  const uint64_t rb = nb0 + base_a[blockIdx.x] + wg_excl(nw, &tb);
  const uint64_t ib = ni0 + base_b[blockIdx.x] + wg_excl(k, &tk);
  if (r >= ncand) return;
  cand_dst[r] = nw ? ib : mvk::IX_NO_SRC;
  if (!nw) return;
  p.slot[rb] = cand_slot[r];
  p.ibase[rb] = ib;
  p.blk[rb] = a.cand_blk[r];
  p.kc[rb] = (uint32_t)k;
}
// one lane per include of the candidates (k_acc_inc_src's shape): its slot into its block's record
__global__ void __launch_bounds__(WG) k_pb_app_inc(AcceptArrays a, uint64_t ncand, uint64_t ninc, const u64* __restrict__ item,
                                                   const uint64_t* __restrict__ cand_dst, PendStore p) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= ninc) return;
  uint64_t lo = 0, hi = ncand;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.inc_base[mid] <= j) lo = mid;
    else hi = mid;
  }
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
__global__ void __launch_bounds__(WG) k_pb_count(const uint8_t* __restrict__ hit, uint64_t nb, uint64_t* __restrict__ wgcount) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(b < nb && hit[b], &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(WG) k_pb_list(u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                const uint8_t* __restrict__ hit, const uint64_t* __restrict__ wgbase,
                                                uint32_t* __restrict__ lvl, uint64_t level, uint64_t* __restrict__ out,
                                                uint64_t cap, u64* __restrict__ ctl, uint32_t* __restrict__ row_of) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool h = b < nb && hit[b];
  uint64_t tot;
  const uint64_t r = wgbase[blockIdx.x] + wg_excl(h, &tot);
  if (h) {
    u64* slot = slots + SLOT_WORDS * p.slot[b];
    lvl[b] = (uint32_t)level + 1;
    if (row_of) row_of[b] = (uint32_t)r;  // (with a DAG store: its record order is the row order)
    if (r < cap) {
#pragma unroll
      for (int w = 0; w < 6; w++) out[8 * r + w] = slot[2 + w];  // (the key: written by an earlier launch)
      out[8 * r + 6] = p.blk[b];
      out[8 * r + 7] = level;
    }
    atomicMax(meta_of(slot), (uint32_t)MV_REF_STORED);
  }
  wave_count_to(ctl + mvk::IX_CTL_STORED, h);
}

// compaction: the records whose own reference is not STORED stay, in order
__device__ inline bool pend_keep(const u64* slots, const PendStore& p, uint64_t nb, uint64_t b, uint64_t* k) {
  const bool keep = b < nb && slot_state(slots, p.slot[b]) != MV_REF_STORED;
  *k = keep ? p.kc[b] : 0;
  return keep;
}
__global__ void __launch_bounds__(WG) k_pb_keep_count(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                      uint64_t* __restrict__ wg_a, uint64_t* __restrict__ wg_b) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t k, tb, tk;
  const bool keep = pend_keep(slots, p, nb, b, &k);
  (void)wg_excl(keep, &tb);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}
__global__ void __launch_bounds__(WG) k_pb_keep_list(const u64* __restrict__ slots, PendStore p, PendStore q, uint64_t nb,
                                                     const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b,
                                                     uint64_t* __restrict__ newbase, uint8_t* __restrict__ state,
                                                     uint64_t n_state) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t k, tb, tk;
  const bool keep = pend_keep(slots, p, nb, b, &k);
  const uint64_t rb = base_a[blockIdx.x] + wg_excl(keep, &tb);
  const uint64_t ib = base_b[blockIdx.x] + wg_excl(k, &tk);
  if (b >= nb) return;
  newbase[b] = keep ? ib : mvk::IX_NO_SRC;
  if (!keep) return;
  q.slot[rb] = p.slot[b];
  q.ibase[rb] = ib;
  q.blk[rb] = mvk::IX_NO_SRC;  // the next call finds it suspended by an earlier one
  q.kc[rb] = p.kc[b];
  if (p.blk[b] < n_state) state[p.blk[b]] = MV_ACC_SUSPENDED;  // (n_state is 0 without a state array)
}
__global__ void __launch_bounds__(WG) k_pb_keep_inc(PendStore p, PendStore q, uint64_t nb, const uint64_t* __restrict__ newbase) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (b >= nb || newbase[b] == mvk::IX_NO_SRC) return;
  const uint64_t from = p.ibase[b], to = newbase[b];
  const uint32_t kc = p.kc[b];
  for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) q.inc[to + i] = p.inc[from + i];
}

// after k_ix_rebuild: slot numbers of the old table become those of the same keys in the new one
// (read-only probes of a table that an earlier launch filled)
__global__ void __launch_bounds__(WG) k_pb_reresolve(const u64* __restrict__ old, IndexTable t, uint64_t* __restrict__ slotidx,
                                                     uint64_t n, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < n) {
    const u64* src = old + SLOT_WORDS * slotidx[i];
    uint64_t k[6], start, tag;
#pragma unroll
    for (int w = 0; w < 6; w++) k[w] = src[2 + w];
    hash_key(t, k, &start, &tag);
    uint64_t p = start, dist = 0;
    fail = true;
    for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
      const u64* slot = t.slots + SLOT_WORDS * p;
      const u64 g = slot[0];
      if (g == 0) break;
      if (g == tag && key_eq(slot, k)) {
        slotidx[i] = p;
        fail = false;
        break;
      }
    }
    probe = (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull);
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
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
  const uint64_t nwg = index_groups(ncand);
  const WgScan w = wg_scan_of(wg, ncand);
  const dim3 g(grid_of(ncand)), b(WG);
  hipLaunchKernelGGL(k_pb_app_count, g, b, 0, s, a, ncand, w.count_a, w.count_b);
  (void)launch_index_scan(w.count_a, nwg, w.base_a, ctl + IX_CTL_PB_NB, nullptr, s);
  (void)launch_index_scan(w.count_b, nwg, w.base_b, ctl + IX_CTL_PB_NI, nullptr, s);
  hipLaunchKernelGGL(k_pb_app_list, g, b, 0, s, a, ncand, cand_slot, w.base_a, w.base_b, p, nb0, ni0, cand_dst);
  if (ninc) hipLaunchKernelGGL(k_pb_app_inc, dim3(grid_of(ninc)), b, 0, s, a, ncand, ninc, (const u64*)item, cand_dst, p);
  return hipGetLastError();
}

hipError_t launch_pend_level(const IndexTable& t, const PendStore& p, uint64_t nb, uint32_t* lvl, uint8_t* hit,
                             uint64_t level, uint64_t* wg, uint64_t* out, uint64_t cap, uint64_t* ctl, int lv_word,
                             uint32_t* row_of, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const WgScan w = wg_scan_of(wg, nb);
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_pb_check, dim3(grid_of(64 * nb)), b, 0, s, (const u64*)t.slots, p, nb, lvl, hit);
  hipLaunchKernelGGL(k_pb_count, g, b, 0, s, hit, nb, w.count_a);
  (void)launch_index_scan(w.count_a, index_groups(nb), w.base_a, ctl + lv_word, ctl + IX_CTL_PB_ROWS, s);
  hipLaunchKernelGGL(k_pb_list, g, b, 0, s, (u64*)t.slots, p, nb, hit, w.base_a, lvl, level, out, cap, (u64*)ctl, row_of);
  return hipGetLastError();
}

hipError_t launch_pend_compact(const IndexTable& t, const PendStore& p, const PendStore& q, uint64_t nb, uint64_t* newbase,
                               uint8_t* state, uint64_t n_state, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  const WgScan w = wg_scan_of(wg, nb);
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_pb_keep_count, g, b, 0, s, (const u64*)t.slots, p, nb, w.count_a, w.count_b);
  (void)launch_index_scan(w.count_a, nwg, w.base_a, ctl + IX_CTL_PB_NB, nullptr, s);
  (void)launch_index_scan(w.count_b, nwg, w.base_b, ctl + IX_CTL_PB_NI, nullptr, s);
  hipLaunchKernelGGL(k_pb_keep_list, g, b, 0, s, (const u64*)t.slots, p, q, nb, w.base_a, w.base_b, newbase, state, state ? n_state : 0);
  hipLaunchKernelGGL(k_pb_keep_inc, dim3(grid_of(64 * nb)), b, 0, s, p, q, nb, newbase);
  return hipGetLastError();
}

hipError_t launch_pend_reresolve(const uint64_t* old_slots, const IndexTable& t, uint64_t* slotidx, uint64_t n,
                                 uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_reresolve, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)old_slots, t, slotidx, n, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
