// The device-resident index of block references (include/mysti_verify.h: mv_index_*,
// mv_accept_blocks, mv_connect_blocks): a set of BlockReferences with a state each -- MV_REF_HAVE,
// what BlockManager::exists_or_pending answers (block_manager.rs:142-144), MV_REF_STORED, what
// BlockStore::block_exists answers, or MV_REF_WANTED, a key of
// block_references_waiting that is not pending (BlockManager::missing, :90-97) -- and the kernels
// of one accept call around the block pipeline (process_blocks' skip, net_sync.rs:325-336, and the
// include lookups of add_blocks, block_manager.rs:62-98). Where references lie in a block:
// block_ref.h.
// The table's layout, the insert protocol and the memory model of every kernel here: index_dev.h.
#include "index_dev.h"

namespace mv::ix {

// wgbase[g] = the counts of the workgroups before g; *total = all of them.
// With `running` (the connect sweep's rows so far): the bases stand behind *running; *running += *total
__global__ void __launch_bounds__(1024) k_ix_scan(const uint64_t* __restrict__ wgcount, uint64_t nwg,
                                                  uint64_t* __restrict__ wgbase, uint64_t* __restrict__ total,
                                                  uint64_t* __restrict__ running) {
  __shared__ uint64_t part[1024];
  const uint64_t before = running ? *running : 0;  // (written below by one lane, after every barrier)
  const uint64_t per = (nwg + 1023) / 1024;
  const uint64_t lo = per * threadIdx.x < nwg ? per * threadIdx.x : nwg;
  const uint64_t hi = lo + per < nwg ? lo + per : nwg;
  uint64_t sum = 0;
  for (uint64_t g = lo; g < hi; g++) sum += wgcount[g];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t acc = before + part[threadIdx.x] - sum;
  for (uint64_t g = lo; g < hi; g++) {
    wgbase[g] = acc;
    acc += wgcount[g];
  }
  if (threadIdx.x == 1023) {
    *total = part[1023];
    if (running) *running = before + part[1023];
  }
}

// ---------------------------------------------------------------- insert rounds
__global__ void __launch_bounds__(WG) k_ix_claim(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                 uint32_t newstate, int round, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool act = i < n;
  if (act && round == 0) {
    act = has_src(ks, i);
    if (!act) item[i] = pack(0, 0, C_NONE);
  } else if (act) {
    act = code_of(item[i]) == C_RETRY;
  }
  uint32_t probe = 0;
  bool fail = false;
  if (act) {
    uint64_t k[6], start, tag;
    load_key(ks, i, k);
    hash_key(t, k, &start, &tag);
    uint64_t p = round ? ((item[i] & SLOT_MASK) + 1) & t.mask : start;
    uint64_t dist = (p - start) & t.mask;  // slots already passed in earlier rounds
    const uint32_t me = ~(uint32_t)i;
    u64 res = pack(0, 0, C_FAIL);
    for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
      u64* slot = t.slots + SLOT_WORDS * p;
      const u64 old = atomicCAS(slot, 0ull, (u64)tag);
      if (old == 0) {
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, 0, C_CLAIMED);
        break;
      }
      if (old != tag) continue;
      const uint32_t st = __hip_atomic_load(meta_of(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (st == 0) {  // claimed in this launch: its key is not there yet
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, 0, C_CLAIMED);
        break;
      }
      if (!key_eq(slot, k)) continue;
      if (st >= newstate) {
        res = pack(p, st, C_NOOP);
      } else {
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, st, C_FOUND);
      }
      break;
    }
    probe = probe_len(dist);
    fail = code_of(res) == C_FAIL;
    item[i] = res;
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

__global__ void __launch_bounds__(WG) k_ix_fill(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                uint32_t newstate, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool created = false, raised = false;
  if (i < n) {
    const u64 it = item[i], c = code_of(it);
    if (c == C_CLAIMED || c == C_FOUND) {
      const uint64_t p = it & SLOT_MASK;
      u64* slot = t.slots + SLOT_WORDS * p;
      uint32_t* meta = meta_of(slot);
      const bool owner = meta[1] == ~(uint32_t)i;  // (set by k_ix_claim's atomics, an earlier kernel)
      if (c == C_CLAIMED && owner) {
        uint64_t k[6];
        load_key(ks, i, k);
#pragma unroll
        for (int w = 0; w < 6; w++) slot[2 + w] = k[w];
        atomicMax(meta, newstate);
        created = true;
        item[i] = pack(p, 0, C_NEW) | FRESH;
      } else if (c == C_FOUND) {
        if (owner) {
          atomicMax(meta, newstate);
          raised = true;
          item[i] = pack(p, prior_of(it), C_RAISED) | FRESH;
        } else {
          item[i] = pack(p, prior_of(it), C_DUP);
        }
      }
    }
  }
  // raises: WANTED -> HAVE, and WANTED or HAVE -> STORED (the HAVE counter holds HAVE and STORED)
  if (newstate >= MV_REF_HAVE) {
    const uint32_t prior = i < n ? prior_of(item[i]) : 0;  // (0 for an entry created now)
    wave_count_to(ctl + mvk::IX_CTL_HAVE, created || (raised && prior < MV_REF_HAVE));
    wave_count_to(ctl + mvk::IX_CTL_WANTED, raised && prior == MV_REF_WANTED, true);
    if (newstate == MV_REF_STORED) wave_count_to(ctl + mvk::IX_CTL_STORED, created || raised);
  } else {
    wave_count_to(ctl + mvk::IX_CTL_WANTED, created);
  }
}

__global__ void __launch_bounds__(WG) k_ix_settle(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                  u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool retry = false;
  if (i < n) {
    const u64 it = item[i];
    const uint64_t p = it & SLOT_MASK;
    u64* slot = t.slots + SLOT_WORDS * p;
    if (code_of(it) == C_CLAIMED) {  // not the owner: the owner's key is there since k_ix_fill
      uint64_t k[6];
      load_key(ks, i, k);
      retry = !key_eq(slot, k);
      item[i] = pack(p, 0, retry ? C_RETRY : C_DUP);
    } else if (it & FRESH) {
      meta_of(slot)[1] = 0;
      item[i] = it & ~FRESH;
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_RETRY, retry);
}

// after the last round a call enqueued ahead: items still left over are given up (the error word)
__global__ void k_ix_giveup(u64* __restrict__ ctl) {
  if (threadIdx.x || blockIdx.x) return;
  if (ctl[mvk::IX_CTL_RETRY]) atomicAdd(ctl + mvk::IX_CTL_ERR, ctl[mvk::IX_CTL_RETRY]);
}

__global__ void __launch_bounds__(WG) k_ix_prior(const u64* __restrict__ item, uint64_t n, uint8_t* __restrict__ prior) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i < n) prior[i] = (uint8_t)prior_of(item[i]);
}

__global__ void __launch_bounds__(WG) k_ix_lookup(IndexTable t, IndexKeys ks, uint64_t n, uint8_t* __restrict__ out,
                                                  u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < n) {
    uint32_t st = MV_REF_ABSENT;
    if (t.slots && has_src(ks, i)) {
      uint64_t k[6];
      load_key(ks, i, k);
      st = lookup(t, k, &probe, &fail);
    }
    out[i] = (uint8_t)st;
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// One lane per slot of the old table: its entry into the new one. The keys are distinct, so a
// lane claims the first empty slot and never compares (no key of this launch is read).
__global__ void __launch_bounds__(WG) k_ix_rebuild(const u64* __restrict__ old, uint64_t old_slots, IndexTable t,
                                                   u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < old_slots) {
    const u64* src = old + SLOT_WORDS * i;
    const uint32_t st = (uint32_t)src[1];
    if (src[0] != 0 && st != 0) {
      uint64_t k[6];
#pragma unroll
      for (int w = 0; w < 6; w++) k[w] = src[2 + w];
      fail = claim_fresh(t, k, st, &probe) == DG_NO_SLOT;
    }
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// After k_ix_rebuild: the slot numbers a store holds (records, includes, queue entries) become
// those of the same keys in the new table, by read-only probes of a table that an earlier launch
// filled. DG_NO_SLOT stays; a number outside the old table, or a key without an entry, becomes
// DG_NO_SLOT and counts into the error word. The probe length is reported, though it tells nothing
// new: a key is found at exactly the slot where k_ix_rebuild placed it, and k_ix_rebuild reported
// that probe length on the same stream.
__global__ void __launch_bounds__(WG) k_ix_reresolve(const u64* __restrict__ old, uint64_t n_old, IndexTable t,
                                                     uint64_t* __restrict__ slotidx, uint64_t n, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool bad = false;
  if (i < n && slotidx[i] != DG_NO_SLOT) {
    const uint64_t o = slotidx[i];
    u64 s = DG_NO_SLOT;
    if (o < n_old) {
      uint64_t k[6];
#pragma unroll
      for (int w = 0; w < 6; w++) k[w] = old[SLOT_WORDS * o + 2 + w];
      s = find_slot(t, k, &probe, &bad);
    }
    bad = s == DG_NO_SLOT;
    slotidx[i] = s;
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// The WANTED entries, listed in slot order
struct WantedList {
  static constexpr int WEIGHTS = 1;
  const u64* slots;
  uint64_t n;
  uint64_t* out;
  uint64_t cap;
  __device__ void weigh(uint64_t i, uint64_t* w) const {
    *w = i < n && slots[SLOT_WORDS * i] != 0 && (uint32_t)slots[SLOT_WORDS * i + 1] == MV_REF_WANTED;
  }
  __device__ void place(uint64_t i, uint64_t w, uint64_t r) const {
    if (w && r < cap) copy_key(out + 6 * r, slots + SLOT_WORDS * i);
  }
};

// ---------------------------------------------------------------- the accept call

__device__ inline bool block_inside(const AcceptArrays& a, uint64_t i) {
  return a.off[i] <= a.buf_bytes && a.len[i] <= a.buf_bytes - a.off[i];
}

// KNOWN: the block's own reference is HAVE or STORED in the index as it stands (net_sync.rs:325-336);
// counts the blocks that go on to verify per workgroup
__global__ void __launch_bounds__(WG) k_acc_probe(IndexTable t, AcceptArrays a, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false, known = false;
  if (i < a.n) {
    const uint64_t len = a.len[i];
    if (t.slots && block_inside(a, i) && br::own_ref_readable(len)) {
      const uint8_t* p = a.buf + a.off[i];
      if (ld64(p + br::LEN_WORD_OFF) == br::DIGEST_LEN) {
        uint64_t k[6];
#pragma unroll
        for (int w = 0; w < 6; w++) k[w] = ld64(p + br::key_word_off(w));
        known = lookup(t, k, &probe, &fail) >= MV_REF_HAVE;
      }
    }
    a.known[i] = known;
  }
  uint64_t tot;
  (void)wg_excl(i < a.n && !known, &tot);
  if (threadIdx.x == 0) a.wg_a[blockIdx.x] = tot;
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// the blocks to verify, in order
__global__ void __launch_bounds__(WG) k_acc_vlist(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool v = i < a.n && !a.known[i];
  uint64_t tot;
  const uint64_t r = a.base_a[blockIdx.x] + wg_excl(v, &tot);
  if (!v) return;
  a.v_off[r] = a.off[i];
  a.v_len[r] = a.len[i];
  a.rank[i] = (uint32_t)r;
}

__device__ inline bool group_head(const AcceptArrays& a, uint64_t i) {
  return i < a.n && (i == 0 || a.grp[i] != a.grp[i - 1]);
}
// the heads per workgroup (count and scan only: k_acc_groups ranks for itself, a head counts itself in)
struct GroupHeads {
  static constexpr int WEIGHTS = 1;
  AcceptArrays a;
  __device__ void weigh(uint64_t i, uint64_t* w) const { *w = group_head(a, i); }
};

// statuses (KNOWN blocks are MV_BLOCK_OK unverified), the group of every block, and a reject flag
// per group: one rejected block drops its message before add_blocks (net_sync.rs:352-361)
__global__ void __launch_bounds__(WG) k_acc_groups(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t g = i;
  if (a.grp) {
    const bool head = group_head(a, i);
    uint64_t tot;
    g = a.base_a[blockIdx.x] + wg_excl(head, &tot) + head - 1;  // heads up to and including i, less one
  }
  if (i >= a.n) return;
  const bool known = a.known[i];
  const uint8_t st = known ? (uint8_t)MV_BLOCK_OK : a.v_status[a.rank[i]];
  a.status[i] = st;
  a.gidx[i] = (uint32_t)g;
  if (!known && st != MV_BLOCK_OK) atomicMax(a.gflag + g, 1u);
}

// states before the duplicates are told apart (candidates are MV_ACC_NEW for now), the include
// count of every candidate, and the per-workgroup counts of both
__global__ void __launch_bounds__(WG) k_acc_states(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool cand = false;
  uint64_t k = 0;
  if (i < a.n) {
    uint8_t s;
    if (a.known[i]) s = MV_ACC_KNOWN;
    else if (a.status[i] != MV_BLOCK_OK) s = MV_ACC_REJECTED;
    else if (a.gflag[a.gidx[i]]) s = MV_ACC_DROPPED;
    else s = MV_ACC_NEW, cand = true;
    // (a block that parsed holds its own reference and its includes; checked again all the same)
    const uint64_t len = a.len[i];
    if (cand && !(block_inside(a, i) && br::own_ref_readable(len))) s = MV_ACC_REJECTED, cand = false;
    if (cand && br::inc_count_readable(len)) {
      k = ld64(a.buf + a.off[i] + br::INC_COUNT_OFF);
      if (!br::includes_inside(len, k)) k = 0;
    }
    a.state[i] = s;
    a.kc[i] = (uint32_t)k;
  }
  uint64_t tc, tk;
  (void)wg_excl(cand, &tc);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    a.wg_a[blockIdx.x] = tc;
    a.wg_b[blockIdx.x] = tk;
  }
}

// the candidates in block order: block, where its own reference lies, its first include's number
__global__ void __launch_bounds__(WG) k_acc_cand_list(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool cand = i < a.n && a.state[i] == MV_ACC_NEW;
  const uint64_t k = cand ? a.kc[i] : 0;
  uint64_t tc, tk;
  const uint64_t r = a.base_a[blockIdx.x] + wg_excl(cand, &tc);
  const uint64_t ib = a.base_b[blockIdx.x] + wg_excl(k, &tk);
  if (!cand) return;
  a.cand_blk[r] = (uint32_t)i;
  a.cand_src[r] = a.off[i];
  a.inc_base[r] = ib;
}

// the lowest block of every reference is NEW, the others DUP (block_manager.rs:68-72)
__global__ void __launch_bounds__(WG) k_acc_own_states(AcceptArrays a, const u64* __restrict__ item, uint64_t ncand) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (r >= ncand) return;
  const u64 c = code_of(item[r]);
  a.state[a.cand_blk[r]] = (c == C_NEW || c == C_RAISED) ? MV_ACC_NEW : MV_ACC_DUP;
}

// one lane per include of the candidates: where it lies, or IX_NO_SRC when its block is not NEW
__global__ void __launch_bounds__(WG) k_acc_inc_src(AcceptArrays a, uint64_t ncand, uint64_t ninc,
                                                    uint64_t* __restrict__ inc_src) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= ninc) return;
  const uint64_t lo = cand_of_include(a.inc_base, ncand, j);
  const uint64_t q = j - a.inc_base[lo];
  const bool is_new = a.state[a.cand_blk[lo]] == MV_ACC_NEW && q < a.kc[a.cand_blk[lo]];
  inc_src[j] = is_new ? a.cand_src[lo] + br::include_off(q) : mvk::IX_NO_SRC;
}

// the includes that created an entry are the missing references, in (block, include) order
struct MissingList {
  static constexpr int WEIGHTS = 1;
  IndexTable t;
  const u64* item;
  uint64_t n;
  uint64_t* out;
  uint64_t cap;
  __device__ void weigh(uint64_t j, uint64_t* w) const { *w = j < n && code_of(item[j]) == C_NEW; }
  __device__ void place(uint64_t j, uint64_t w, uint64_t r) const {
    if (w && r < cap) copy_key(out + 6 * r, t.slots + SLOT_WORDS * (item[j] & SLOT_MASK));
  }
};

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_index_scan(const uint64_t* wgcount, uint64_t nwg, uint64_t* wgbase, uint64_t* total, uint64_t* running,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wgcount, nwg, wgbase, total, running);
  return hipPeekAtLastError();  // (left standing for the hipGetLastError that ends every launcher)
}

hipError_t launch_index_round(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint64_t* item, uint32_t state,
                              int round, uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  u64* c = (u64*)ctl;
  const dim3 g(grid_of(n)), b(WG);
  hipLaunchKernelGGL(k_ix_claim, g, b, 0, s, t, ks, n, (u64*)item, state, round, c);
  hipLaunchKernelGGL(k_ix_fill, g, b, 0, s, t, ks, n, (u64*)item, state, c);
  hipLaunchKernelGGL(k_ix_settle, g, b, 0, s, t, ks, n, (u64*)item, c);
  return hipGetLastError();
}

hipError_t launch_index_giveup(uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_ix_giveup, dim3(1), dim3(64), 0, s, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_prior(const uint64_t* item, uint64_t n, uint8_t* prior, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_prior, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)item, n, prior);
  return hipGetLastError();
}

hipError_t launch_index_lookup(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint8_t* out, uint64_t* ctl,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_lookup, dim3(grid_of(n)), dim3(WG), 0, s, t, ks, n, out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_rebuild(const uint64_t* old_slots, uint64_t n_old, const IndexTable& t, uint64_t* ctl,
                                hipStream_t s) {
  if (n_old == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_rebuild, dim3(grid_of(n_old)), dim3(WG), 0, s, (const u64*)old_slots, n_old, t, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_reresolve(const uint64_t* old_slots, uint64_t n_old, const IndexTable& t, uint64_t* slotidx,
                                  uint64_t n, uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_reresolve, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)old_slots, n_old, t, slotidx, n, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_wanted(const IndexTable& t, uint64_t* wg, uint64_t* total, uint64_t* out, uint64_t cap,
                               hipStream_t s) {
  const uint64_t n = t.mask + 1;
  compact_pass(WantedList{(const u64*)t.slots, n, out, cap}, n, wg_scan_of(wg, n), total, nullptr, nullptr, s, cap != 0);
  return hipGetLastError();
}

hipError_t launch_accept_probe(const IndexTable& t, const AcceptArrays& a, uint64_t* ctl, hipStream_t s) {
  const dim3 g(grid_of(a.n)), b(WG);
  hipLaunchKernelGGL(k_acc_probe, g, b, 0, s, t, a, (u64*)ctl);
  (void)launch_index_scan(a.wg_a, index_groups(a.n), a.base_a, ctl + IX_CTL_NVER, nullptr, s);
  hipLaunchKernelGGL(k_acc_vlist, g, b, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_accept_groups(const AcceptArrays& a, uint64_t* ctl, hipStream_t s) {
  const dim3 g(grid_of(a.n)), b(WG);
  const uint64_t nwg = index_groups(a.n);
  if (a.grp) compact_count(GroupHeads{a}, a.n, WgScan{a.wg_a, a.wg_b, a.base_a, a.base_b}, ctl + IX_CTL_NHEADS, nullptr, nullptr, s);
  hipLaunchKernelGGL(k_acc_groups, g, b, 0, s, a);
  hipLaunchKernelGGL(k_acc_states, g, b, 0, s, a);
  (void)launch_index_scan(a.wg_a, nwg, a.base_a, ctl + IX_CTL_NCAND, nullptr, s);
  (void)launch_index_scan(a.wg_b, nwg, a.base_b, ctl + IX_CTL_NINC, nullptr, s);
  hipLaunchKernelGGL(k_acc_cand_list, g, b, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_accept_own_states(const AcceptArrays& a, const uint64_t* item, uint64_t ncand, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_acc_own_states, dim3(grid_of(ncand)), dim3(WG), 0, s, a, (const u64*)item, ncand);
  return hipGetLastError();
}

hipError_t launch_accept_inc_src(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, uint64_t* inc_src, hipStream_t s) {
  if (ninc == 0 || ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_acc_inc_src, dim3(grid_of(ninc)), dim3(WG), 0, s, a, ncand, ninc, inc_src);
  return hipGetLastError();
}

hipError_t launch_accept_missing(const IndexTable& t, const uint64_t* item, uint64_t ninc, uint64_t* wg, uint64_t* ctl,
                                 uint64_t* out, uint64_t cap, hipStream_t s) {
  if (ninc == 0) return hipSuccess;
  compact_pass(MissingList{t, (const u64*)item, ninc, out, cap}, ninc, wg_scan_of(wg, ninc), ctl + IX_CTL_NMISS, nullptr,
               nullptr, s, cap != 0);
  return hipGetLastError();
}

}  // namespace mvk
