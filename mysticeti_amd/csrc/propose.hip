// The proposer's state over the index and the DAG store (mv_propose_*): the threshold clock of
// ThresholdClockAggregator::add_block (threshold_clock.rs:58-89), the `pending` queue of Core
// (core.rs:197-198, 223-224) and the include choice of Core::try_new_block (core.rs:232-278); the
// wording of every rule is the header's. The memory model is index_dev.h's: inside one launch lanes
// talk only through agent-scope atomic read-modify-writes on single words (or LDS atomics inside a
// wave), nobody waits, and what a kernel reads as plain data an earlier launch wrote. Every slot,
// record and entry number is checked against its array before it is an address; a failed check counts
// into the error word (MV_E_HIP) and is not followed. Every loop is bounded by a count read under such
// a check.
//   k_pp_resolve   a lane per row: its slot by a probe of the table, its round and authority
//   SortBit        one pass of the stable sort by round (a pass per bit in which the call's rounds
//                  differ): a compaction pass of index_dev.h over the zeros, the ones behind them
//   k_pp_append    a lane per sorted row: its queue entry; the payload entry behind them
//   k_pp_seg       the clock, batch form: a wave per segment of equal round -- which rows are the first
//                  of their author (an LDS table of first rows per authority), the prefix of their
//                  stakes, the first row at which it passes the quorum
//   k_pp_chain     one wave over the segments in order: Less / Greater / Equal per segment from the
//                  round so far; a segment that starts from the empty set is answered by k_pp_seg's
//                  words, one that continues a set is walked 64 rows a step with the set in LDS
//   k_pp_cut       the first include entry at or above the clock round
//   k_pp_stamp     a wave per taken entry (and one for the own last block): lanes over its record's includes
//   KeepEntries    a compaction pass: the unstamped include entries and the payloads, each in queue order
//   k_pp_shift     the tail moves to the front (into the queue's other copy)
//   k_pp_own, k_pp_record   the own last block's slots; its record in the DAG store
// After a rebuild the queue's, the own block's and the choice's slot numbers go through index.hip's k_ix_reresolve.
#include "index_dev.h"

namespace mv::ix {

using mvk::PropClock;
using mvk::PropQueue;

__global__ void __launch_bounds__(WG) k_pp_resolve(IndexTable t, const uint64_t* __restrict__ rows, uint64_t n, uint64_t stride,
                                                   uint32_t n_auth, uint64_t* __restrict__ slot, uint64_t* __restrict__ round,
                                                   uint32_t* __restrict__ auth, uint32_t* __restrict__ perm,
                                                   u64* __restrict__ pctl, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false, miss = false;
  if (i < n) {
    uint64_t k[6];
    for (int w = 0; w < 6; w++) k[w] = rows[stride * i + w];
    uint32_t probe;  // (not reported: this call's probes never were)
    const u64 s = find_slot(t, k, &probe, &bad);
    // (StakeAggregator::add panics on an authority outside the committee, committee.rs:315)
    miss = s == DG_NO_SLOT || k[0] >= n_auth;
    slot[i] = s;
    round[i] = k[1];
    auth[i] = k[0] < n_auth ? (uint32_t)k[0] : DG_NONE;
    perm[i] = (uint32_t)i;
    atomicOr(pctl + mvk::PP_CTL_OR, (u64)k[1]);
    atomicOr(pctl + mvk::PP_CTL_NOR, ~(u64)k[1]);
  }
  wave_count_to(pctl + mvk::PP_CTL_NMISS, miss);
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

struct SortBit {
  static constexpr int WEIGHTS = 1;
  const uint64_t* round;
  int bit;
  const uint32_t* perm;
  uint32_t* out;
  uint64_t n;
  const u64* pctl;
  __device__ void weigh(uint64_t i, uint64_t* zero) const {
    const uint32_t r = i < n ? perm[i] : DG_NONE;
    *zero = r < n && ((round[r] >> bit) & 1) == 0;
  }
  __device__ void place(uint64_t i, uint64_t z, uint64_t zb) const {  // zb: the zeros before i
    if (i >= n) return;
    const uint64_t zeros = pctl[mvk::PP_CTL_ZEROS];  // (the scan, an earlier launch)
    const uint64_t dst = z ? zb : zeros + (i - zb);
    if (dst < n) out[dst] = perm[i];
  }
};

__global__ void __launch_bounds__(WG) k_pp_append(const uint64_t* __restrict__ slot, const uint64_t* __restrict__ round,
                                                  const uint32_t* __restrict__ auth, const uint64_t* __restrict__ tags,
                                                  const uint32_t* __restrict__ perm, uint64_t n, PropQueue q, uint64_t q0,
                                                  uint64_t qcap, uint32_t* __restrict__ sauth, bool payload, uint64_t token,
                                                  u64* __restrict__ ctl) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (j < n) {
    const uint32_t r = perm[j];
    bad = r >= n || q0 + j >= qcap;
    if (!bad) {
      q.kind[q0 + j] = mvk::PP_INCLUDE;
      q.slot[q0 + j] = slot[r];
      q.round[q0 + j] = round[r];
      q.tag[q0 + j] = tags ? tags[r] : 0;
      sauth[j] = auth[r];
    }
  } else if (j == n && payload) {
    bad = q0 + n >= qcap;
    if (!bad) {
      q.kind[q0 + n] = mvk::PP_PAYLOAD;
      q.slot[q0 + n] = DG_NO_SLOT;
      q.round[q0 + n] = 0;
      q.tag[q0 + n] = token;
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// the inclusive prefix of v over the wave
__device__ inline uint64_t wave_incl64(uint64_t v) {
  const uint32_t lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// A wave per row; the wave of a segment's first row does the segment. The LDS table holds, per
// authority, the first row of the segment that names it (an atomic min inside the wave).
__global__ void __launch_bounds__(WG) k_pp_seg(PropClock c) {
  __shared__ uint32_t tab_all[WG / 64][DG_MAX_AUTH];
  const uint64_t i = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;
  const uint32_t lane = threadIdx.x & 63;
  if (i >= c.n) return;
  const uint64_t r = c.round[i];
  if (i > 0 && c.round[i - 1] == r) return;  // not a segment's first row (the whole wave leaves)
  uint32_t* tab = tab_all[threadIdx.x / 64];
  uint64_t e = i;
  while (e < c.n) {  // bounded by the rows: every turn but the last passes 64 of them
    const uint64_t idx = e + lane;
    const u64 m = __ballot(idx < c.n && c.round[idx] == r);
    const uint32_t cnt = m == ~0ull ? 64u : (uint32_t)__ffsll((long long)~m) - 1;
    e += cnt;
    if (cnt < 64) break;
  }
  const uint64_t len = e - i;  // (at least 1, below 2^32: the rows of a call are)
  for (uint32_t a = lane; a < DG_MAX_AUTH; a += 64) tab[a] = DG_NONE;
  wave_sync();
  for (uint64_t o = lane; o < len; o += 64) {
    const uint32_t a = c.auth[i + o];
    if (a < c.n_auth && a < DG_MAX_AUTH) atomicMin(tab + a, (uint32_t)o);
  }
  wave_sync();
  uint64_t carry = 0;
  uint32_t pos0 = DG_NONE, pos1 = DG_NONE;
  for (uint64_t o0 = 0; o0 < len; o0 += 64) {  // the wave stays together
    const uint64_t o = o0 + lane;
    uint64_t w = 0;
    if (o < len) {
      const uint32_t a = c.auth[i + o];
      const bool f = a < c.n_auth && a < DG_MAX_AUTH && tab[a] == (uint32_t)o;
      c.first[i + o] = f;
      w = f ? c.stakes[a] : 0;
    }
    const uint64_t pre = carry + wave_incl64(w);
    const u64 hit = __ballot(o < len && pre > c.quorum);
    if (hit && pos0 == DG_NONE) pos0 = (uint32_t)(o0 + __ffsll((long long)hit) - 1);
    const u64 hit1 = o0 ? hit : hit & ~1ull;
    if (hit1 && pos1 == DG_NONE) pos1 = (uint32_t)(o0 + __ffsll((long long)hit1) - 1);
    carry = shfl64(pre, 63);
  }
  if (lane == 0) {
    c.seglen[i] = (uint32_t)len;
    c.pos0[i] = pos0;
    c.pos1[i] = pos1;
    c.stot[i] = carry;
  }
}

// One wave, every lane on the same path (what decides a branch is read by all lanes alike).
__global__ void __launch_bounds__(64) k_pp_chain(PropClock c, u64* __restrict__ pctl, u64* __restrict__ ctl) {
  __shared__ uint32_t V[DG_BM];
  const uint32_t lane = threadIdx.x;
  uint64_t R = pctl[mvk::PP_CTL_ROUND], S = pctl[mvk::PP_CTL_STAKE];
  const uint32_t* bm = reinterpret_cast<const uint32_t*>(pctl + mvk::PP_CTL_BM);
  if (lane < (uint32_t)DG_BM) V[lane] = bm[lane];
  wave_sync();
  bool empty = pctl[mvk::PP_CTL_VOTERS] == 0, bad = false;
  for (uint64_t i = 0; i < c.n;) {  // bounded by the rows: a segment has at least one
    const uint64_t r = c.round[i], len = c.seglen[i];
    if (len == 0 || len > c.n - i) {
      bad = true;
      break;
    }
    if (r >= R) {
      const bool greater = r > R;
      if (greater || empty) {
        // from the empty set: Greater adds the first row without asking (threshold_clock.rs:63-67)
        const uint32_t p = greater ? c.pos1[i] : c.pos0[i];
        if (p != DG_NONE) {
          R = r + 1, S = 0, empty = true;
          if (lane < (uint32_t)DG_BM) V[lane] = 0;
          wave_sync();
        } else {
          if (lane < (uint32_t)DG_BM) V[lane] = 0;
          wave_sync();
          for (uint64_t o = lane; o < len; o += 64) {
            const uint32_t a = c.auth[i + o];
            if (c.first[i + o] && a < DG_MAX_AUTH) atomicOr(V + (a >> 5), 1u << (a & 31));
          }
          wave_sync();
          R = r, S = c.stot[i], empty = false;
        }
      } else {
        // Equal, continuing a set: the rows 64 a step, the set read before the step's authors join it
        bool done = false;
        for (uint64_t o0 = 0; o0 < len && !done; o0 += 64) {
          const uint64_t o = o0 + lane;
          uint32_t a = DG_NONE;
          bool isnew = false;
          if (o < len) {
            a = c.auth[i + o];
            isnew = c.first[i + o] && a < DG_MAX_AUTH && a < c.n_auth && !((V[a >> 5] >> (a & 31)) & 1u);
          }
          const uint64_t pre = S + wave_incl64(isnew ? c.stakes[a] : 0);
          const u64 hit = __ballot(o < len && pre > c.quorum);
          wave_sync();
          if (hit) {
            R = r + 1, S = 0, empty = true, done = true;
            if (lane < (uint32_t)DG_BM) V[lane] = 0;
          } else {
            if (isnew) atomicOr(V + (a >> 5), 1u << (a & 31));
            S = shfl64(pre, 63);
          }
          wave_sync();
        }
      }
    }
    i += len;
  }
  uint32_t voters = lane < (uint32_t)DG_BM ? (uint32_t)__popc(V[lane]) : 0;
  for (int d = 32; d; d >>= 1) voters += (uint32_t)__shfl_xor((int)voters, d);
  uint32_t* out = reinterpret_cast<uint32_t*>(pctl + mvk::PP_CTL_BM);
  if (lane < (uint32_t)DG_BM) out[lane] = V[lane];
  if (lane == 0) {
    pctl[mvk::PP_CTL_ROUND] = R;
    pctl[mvk::PP_CTL_STAKE] = S;
    pctl[mvk::PP_CTL_VOTERS] = voters;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && lane == 0);
}

__global__ void __launch_bounds__(WG) k_pp_cut(PropQueue q, uint64_t qn, uint64_t round, u64* __restrict__ pctl) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const u64 m = __ballot(j < qn && q.kind[j] == mvk::PP_INCLUDE && q.round[j] >= round);
  if ((threadIdx.x & 63) == 0 && m) atomicMin(pctl + mvk::PP_CTL_CUT, (u64)(j + __ffsll((long long)m) - 1));
}

__global__ void __launch_bounds__(WG) k_pp_stamp(PropQueue q, uint64_t cut, DagStore d, uint64_t nb, bool dag_on,
                                                 const uint64_t* __restrict__ own_inc, uint64_t n_own,
                                                 uint32_t* __restrict__ stamp, uint64_t n_stamp, uint32_t counter,
                                                 u64* __restrict__ pctl, u64* __restrict__ ctl) {
  const uint64_t j = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per taken entry, one more for the own block
  const uint32_t lane = threadIdx.x & 63;
  if (j > cut) return;
  const uint64_t* inc = nullptr;
  uint64_t kc = 0;
  bool bad = false;
  if (j == cut) {
    inc = own_inc, kc = n_own;
  } else if (q.kind[j] == mvk::PP_INCLUDE) {
    const uint64_t s = q.slot[j];
    uint32_t rec = DG_NONE;
    if (s >= n_stamp) bad = true;
    else if (dag_on && s < d.n_slots) rec = d.map[s];
    if (!bad && rec == DG_NONE) {
      // BlockStore::get_block gives None (core.rs:259): nothing joins the set
      if (q.round[j] != 0 && lane == 0) atomicOr(pctl + mvk::PP_CTL_FLAGS, (u64)MV_PROPOSE_INCOMPLETE);
    } else if (!bad) {
      if (rec >= nb) {
        bad = true;
      } else {
        const uint64_t base = d.ibase[rec];
        kc = d.kc[rec];
        bad = base > d.cap_i || kc > d.cap_i - base;
        if (bad) kc = 0;
        else inc = d.inc + base;
      }
    }
  }
  uint64_t nbad = bad && lane == 0;
  for (uint64_t o = lane; o < kc; o += 64) {  // bounded by the include count
    const uint64_t s = inc[o];
    if (s < n_stamp) stamp[s] = counter;  // (plain stores of one value: no lane reads a stamp in this launch)
    else nbad++;
  }
  nbad = wave_sum64(nbad);
  if (lane == 0 && nbad) atomicAdd(ctl + mvk::IX_CTL_ERR, (u64)nbad);
}

// the include entries below the cut that no stamp reached stay; weights: such an entry, a payload entry
struct KeepEntries {
  static constexpr int WEIGHTS = 2;
  const u64* slots;
  PropQueue q;
  uint64_t qn, cut;
  const uint32_t* stamp;
  uint64_t n_stamp;
  uint32_t counter;
  uint64_t* includes;
  uint64_t cap;
  uint64_t* choice;
  uint64_t cap_choice;
  uint64_t* payloads;
  uint64_t cap_p;
  u64* pctl;
  __device__ void weigh(uint64_t j, uint64_t* keep, uint64_t* pay) const {
    *keep = *pay = 0;
    if (j >= cut) return;
    const uint32_t kind = q.kind[j];
    *pay = kind == mvk::PP_PAYLOAD;
    if (kind != mvk::PP_INCLUDE) return;
    const uint64_t s = q.slot[j];
    *keep = s < n_stamp && stamp[s] != counter;  // (a slot outside the table: k_pp_stamp counted it)
  }
  __device__ void place(uint64_t j, uint64_t keep, uint64_t ra, uint64_t pay, uint64_t rb) const {
    if (keep) {
      const uint64_t s = q.slot[j];  // (below n_stamp, the table's size: weigh)
      if (ra < cap) copy_key(includes + 6 * ra, slots + SLOT_WORDS * s);
      if (ra < cap_choice) choice[ra] = s;
    }
    if (pay && rb < cap_p) payloads[rb] = q.tag[j];
    if (j == 0) pctl[mvk::PP_CTL_NEXT] = cut < qn ? q.tag[cut] : ~0ull;
    // The include entries below the cut, kept or not: neither weight says it, so the kind is read again.
    // It is counted here, in the list launch: this pass must never run with list = false.
    wave_count_to(pctl + mvk::PP_CTL_NENT, j < cut && q.kind[j] == mvk::PP_INCLUDE);
  }
};

__global__ void __launch_bounds__(WG) k_pp_shift(PropQueue q, PropQueue to, uint64_t cut, uint64_t qn) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= qn - cut) return;
  to.kind[j] = q.kind[cut + j];
  to.slot[j] = q.slot[cut + j];
  to.round[j] = q.round[cut + j];
  to.tag[j] = q.tag[cut + j];
}

__global__ void __launch_bounds__(WG) k_pp_own(const u64* __restrict__ item, const uint64_t* __restrict__ prev, bool has_prev,
                                               const uint64_t* __restrict__ src, uint64_t n_src, uint64_t* __restrict__ own_out,
                                               uint64_t n_slots, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const uint64_t hp = has_prev ? 1 : 0;
  bool bad = false;
  if (i == 0) {
    const u64 it = item[0];
    const uint64_t s = it & SLOT_MASK;
    bad = !item_has_slot(it) || s >= n_slots;
    own_out[0] = bad ? DG_NO_SLOT : s;
  } else if (i == 1 && has_prev) {
    own_out[1] = prev[0];
  } else if (i >= 1 + hp && i - 1 - hp < n_src) {
    own_out[i] = src[i - 1 - hp];
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_pp_record(const u64* __restrict__ slots, DagStore d, uint64_t nb, uint64_t ni,
                                                  const uint64_t* __restrict__ own, uint64_t k, u64* __restrict__ pctl,
                                                  u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const uint64_t s = own[0];
  // every lane decides alike: map[] is as the launches before left it (k_pp_record_map sets it)
  const bool misfit = s >= d.n_slots || nb >= d.cap_b || ni > d.cap_i || k > d.cap_i - ni;
  const bool append = !misfit && d.map[s] == DG_NONE;
  bool bad = misfit && i == 0;
  if (append && i < k) {
    const uint64_t v = own[1 + i];
    bad = v >= d.n_slots;
    d.inc[ni + i] = bad ? DG_NO_SLOT : v;
  }
  if (append && i == 0) {
    const u64* slot = slots + SLOT_WORDS * s;
    const u64 a = slot[2], rd = slot[3];
    d.slot[nb] = s;
    d.auth[nb] = a < DG_MAX_AUTH ? (uint32_t)a : DG_NONE;
    d.round[nb] = rd;
    d.ibase[nb] = ni;
    d.kc[nb] = (uint32_t)k;
    atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
    atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    pctl[mvk::PP_CTL_APPENDED] = 1;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}
// (its own launch: k_pp_record's lanes read map[slot] to decide)
__global__ void __launch_bounds__(64) k_pp_record_map(DagStore d, uint64_t nb, const uint64_t* __restrict__ own,
                                                      const u64* __restrict__ pctl) {
  const uint64_t s = own[0];
  if (threadIdx.x == 0 && pctl[mvk::PP_CTL_APPENDED] && s < d.n_slots && nb < d.cap_b) d.map[s] = (uint32_t)nb;
}

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_propose_resolve(const IndexTable& t, const uint64_t* rows, uint64_t n, uint64_t stride_words, uint32_t n_auth,
                                  uint64_t* slot, uint64_t* round, uint32_t* auth, uint32_t* perm, uint64_t* pctl,
                                  uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pp_resolve, dim3(grid_of(n)), dim3(WG), 0, s, t, rows, n, stride_words, n_auth, slot, round, auth, perm,
                     (u64*)pctl, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_propose_sort_bit(const uint64_t* round, int bit, const uint32_t* perm, uint32_t* perm_out,
                                   uint64_t n, uint64_t* wg, uint64_t* pctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  compact_pass(SortBit{round, bit, perm, perm_out, n, (const u64*)pctl}, n, wg_scan_of(wg, n), pctl + PP_CTL_ZEROS, nullptr,
               nullptr, s);
  return hipGetLastError();
}

hipError_t launch_propose_append(const uint64_t* slot, const uint64_t* round, const uint32_t* auth, const uint64_t* tags,
                                 const uint32_t* perm, uint64_t n, const PropQueue& q, uint64_t q0, uint64_t qcap,
                                 uint32_t* sauth, bool payload, uint64_t token, uint64_t* ctl, hipStream_t s) {
  if (n == 0 && !payload) return hipSuccess;
  hipLaunchKernelGGL(k_pp_append, dim3(grid_of(n + 1)), dim3(WG), 0, s, slot, round, auth, tags, perm, n, q, q0, qcap, sauth,
                     payload, token, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_propose_clock(const PropClock& c, uint64_t* pctl, uint64_t* ctl, hipStream_t s) {
  if (c.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pp_seg, dim3(grid_of(64 * c.n)), dim3(WG), 0, s, c);
  hipLaunchKernelGGL(k_pp_chain, dim3(1), dim3(64), 0, s, c, (u64*)pctl, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_propose_cut(const PropQueue& q, uint64_t qn, uint64_t round, uint64_t* pctl, hipStream_t s) {
  if (qn == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pp_cut, dim3(grid_of(qn)), dim3(WG), 0, s, q, qn, round, (u64*)pctl);
  return hipGetLastError();
}

hipError_t launch_propose_stamp(const PropQueue& q, uint64_t cut, const DagStore& d, uint64_t nb, bool dag_on,
                                const uint64_t* own_inc, uint64_t n_own, uint32_t* stamp, uint64_t n_stamp, uint32_t counter,
                                uint64_t* pctl, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_pp_stamp, dim3(grid_of(64 * (cut + 1))), dim3(WG), 0, s, q, cut, d, nb, dag_on, own_inc, n_own, stamp,
                     n_stamp, counter, (u64*)pctl, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_propose_keep(const IndexTable& t, const PropQueue& q, uint64_t qn, uint64_t cut, const uint32_t* stamp,
                               uint64_t n_stamp, uint32_t counter, uint64_t* includes, uint64_t cap, uint64_t* choice,
                               uint64_t cap_choice, uint64_t* payloads, uint64_t cap_p, uint64_t* wg, uint64_t* pctl,
                               uint64_t* ctl, hipStream_t s) {
  const uint64_t items = cut ? cut : 1;  // (lane 0 also notes the next tag)
  compact_pass(KeepEntries{(const u64*)t.slots, q, qn, cut, stamp, n_stamp, counter, includes, cap, choice, cap_choice, payloads,
                           cap_p, (u64*)pctl},
               items, wg_scan_of(wg, items), pctl + PP_CTL_NINC, pctl + PP_CTL_NPAY, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_propose_shift(const PropQueue& q, const PropQueue& to, uint64_t cut, uint64_t qn, hipStream_t s) {
  if (cut >= qn) return hipSuccess;
  hipLaunchKernelGGL(k_pp_shift, dim3(grid_of(qn - cut)), dim3(WG), 0, s, q, to, cut, qn);
  return hipGetLastError();
}

hipError_t launch_propose_own(const uint64_t* item, const uint64_t* prev, bool has_prev, const uint64_t* src, uint64_t n_src,
                              uint64_t* own_out, uint64_t n_slots, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_pp_own, dim3(grid_of(n_src + 2)), dim3(WG), 0, s, (const u64*)item, prev, has_prev, src, n_src, own_out,
                     n_slots, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_propose_record(const IndexTable& t, const DagStore& d, uint64_t nb, uint64_t ni, const uint64_t* own,
                                 uint64_t k, uint64_t* pctl, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_pp_record, dim3(grid_of(k ? k : 1)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, ni, own, k, (u64*)pctl,
                     (u64*)ctl);
  hipLaunchKernelGGL(k_pp_record_map, dim3(1), dim3(64), 0, s, d, nb, own, (const u64*)pctl);
  return hipGetLastError();
}

}  // namespace mvk
