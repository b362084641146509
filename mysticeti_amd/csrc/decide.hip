// The direct decision rule and the commit sequence over the DAG store (dag_store.hip).
// mv_decide_leaders: BaseCommitter::try_direct_decide at wave length 3 over the stored edges
// (base_committer.rs:228-357; the wording of every predicate is the header's). The memory model is
// index_dev.h's; inside one wave, k_dg_cert collects a bitmap in LDS under wave-scope fences. Every
// slot and record number is checked against the table size and the store's count before it is an address.
//   PickRoles    a lane per record: is it a voting (r + 1) or a decision (r + 2) record of a leader
//                round, by binary search over the sorted distinct rounds; a compaction pass of
//                index_dev.h into vlist and dlist; a leader block adds itself to its rows' candidates
//   k_dg_vote    a wave per (voting record, row of that round): any include of the authority, the
//                first (authority, round) include in include order across batches of 64
//   k_dg_cert    a wave per (decision record, row): the vote authors among its includes per candidate
//   k_dg_decide  a wave per row: stakes of the bitmaps, the status and the row
#include "index_dev.h"

namespace mv::ix {

using mvk::DecideIn;
using mvk::DecideState;

// *g = the place of `round` among the call's distinct leader rounds
__device__ inline bool leader_group(const DecideIn& in, uint64_t round, uint64_t* g) {
  uint64_t lo = 0, hi = in.ng;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (in.g_round[mid] < round) lo = mid + 1;
    else hi = mid;
  }
  *g = lo;
  return lo < in.ng && in.g_round[lo] == round;
}
struct PickRoles {
  static constexpr int WEIGHTS = 2;
  DagStore d;
  uint64_t nb;
  DecideIn in;
  DecideState st;
  __device__ void weigh(uint64_t rec, uint64_t* voting, uint64_t* decision) const {
    uint64_t g;
    const uint64_t rd = rec < nb ? d.round[rec] : 0;
    *voting = rec < nb && rd >= 1 && leader_group(in, rd - 1, &g);
    *decision = rec < nb && rd >= 2 && leader_group(in, rd - 2, &g);
  }
  __device__ void place(uint64_t rec, uint64_t v, uint64_t pv, uint64_t c, uint64_t pc) const {
    if (rec >= nb) return;
    st.vpos[rec] = v && pv < nb ? (uint32_t)pv : DG_NONE;
    if (v && pv < nb) st.vlist[pv] = (uint32_t)rec;
    if (c && pc < nb) st.dlist[pc] = (uint32_t)rec;
    uint64_t g;
    if (!leader_group(in, d.round[rec], &g)) return;
    // a leader block of every row (authority, round) that names it; bounded by the rows of the round
    const uint64_t a = d.auth[rec], hi = in.g_start[g + 1] < in.n ? in.g_start[g + 1] : in.n;
    for (uint64_t k = in.g_start[g]; k < hi; k++) {
      if (in.l_auth[k] != a) continue;
      const uint32_t at = atomicAdd(st.cand_n + k, 1u);
      if (at < DG_CAND) st.cand_slot[DG_CAND * k + at] = d.slot[rec];
    }
  }
};

// which (record of a list, row) a wave works on; false: none
__device__ inline bool wave_task(const DagStore& d, uint64_t nb, const DecideIn& in, const uint32_t* __restrict__ list,
                                 uint64_t n_list, uint64_t back, uint64_t* at, uint64_t* j, uint64_t* rec, uint64_t* k,
                                 bool* bad) {
  const uint64_t w = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // the same for the whole wave
  *at = w / in.gmax, *j = w % in.gmax;
  if (*at >= n_list) return false;
  *rec = list[*at];
  if (*rec >= nb) {
    *bad = true;
    return false;
  }
  const uint64_t rd = d.round[*rec];
  uint64_t g;
  if (rd < back || !leader_group(in, rd - back, &g)) return false;
  *k = in.g_start[g] + *j;
  return *k < in.g_start[g + 1] && *k < in.n;
}

__global__ void __launch_bounds__(WG) k_dg_vote(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                DecideState st, uint64_t nvote, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t vi, j, rec, k;
  bool bad = false;
  if (wave_task(d, nb, in, st.vlist, nvote, 1, &vi, &j, &rec, &k, &bad)) {
    const uint64_t a = in.l_auth[k], r = in.l_round[k];
    const uint64_t base = d.ibase[rec];
    const uint32_t kc = d.kc[rec];
    bad = base > d.cap_i || kc > d.cap_i - base;
    if (!bad) {
      bool any = false;
      u64 sup = DG_NO_SLOT;
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
        const uint32_t q = q0 + lane;
        u64 s = DG_NO_SLOT;
        bool has_a = false, match = false;
        if (q < kc) {
          s = d.inc[base + q];
          if (s < d.n_slots) {
            has_a = slots[SLOT_WORDS * s + 2] == a;  // the authority only (base_committer.rs:234-237)
            match = has_a && slots[SLOT_WORDS * s + 3] == r;
          } else {
            bad = true;
          }
        }
        any = any || __ballot(has_a) != 0;
        const u64 m = __ballot(match);
        if (m && sup == DG_NO_SLOT) sup = shfl64(s, __ffsll((long long)m) - 1);  // the first in include order
      }
      const uint32_t author = d.auth[rec];
      if (lane == 0) {
        st.sup[vi * in.gmax + j] = sup;
        if (author < DG_MAX_AUTH) {
          const uint32_t bit = 1u << (author & 31);
          if (!any) atomicOr(st.blame + DG_BM * k + (author >> 5), bit);
          const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
          for (uint32_t c = 0; c < cn; c++)
            if (sup != DG_NO_SLOT && st.cand_slot[DG_CAND * k + c] == sup)
              atomicOr(st.vote + DG_BM * (DG_CAND * k + c) + (author >> 5), bit);
        }
      }
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_dg_cert(DagStore d, uint64_t nb, DecideIn in, DecideState st, uint64_t nvote,
                                                uint64_t ndec, const uint64_t* __restrict__ stakes, uint32_t n_auth,
                                                uint64_t quorum_thr, u64* __restrict__ ctl) {
  __shared__ uint32_t bms[WG / 64][DG_CAND][DG_BM];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t(*bm)[DG_BM] = bms[threadIdx.x / 64];
  uint64_t di, j, rec, k;
  bool bad = false;
  if (wave_task(d, nb, in, st.dlist, ndec, 2, &di, &j, &rec, &k, &bad)) {
    const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
    const uint32_t author = d.auth[rec];
    const uint64_t base = d.ibase[rec], vround = d.round[rec] - 1;
    const uint32_t kc = d.kc[rec];
    bad = base > d.cap_i || kc > d.cap_i - base;
    if (!bad && cn && author < n_auth && author < DG_MAX_AUTH) {
      for (uint32_t i = lane; i < DG_CAND * DG_BM; i += 64) (&bm[0][0])[i] = 0;
      wave_sync();
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {
        const uint32_t q = q0 + lane;
        if (q >= kc) continue;
        const u64 s = d.inc[base + q];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        const uint32_t v = d.map[s];  // an include without a record (seeded, pruned) votes for nothing
        if (v == DG_NONE) continue;
        if (v >= nb) {
          bad = true;
          continue;
        }
        const uint32_t va = d.auth[v], vp = st.vpos[v];
        if (d.round[v] != vround || va >= n_auth || va >= DG_MAX_AUTH || vp >= nvote) continue;
        const u64 sup = st.sup[(uint64_t)vp * in.gmax + j];  // (k_dg_vote's, an earlier launch)
        if (sup == DG_NO_SLOT) continue;
        for (uint32_t c = 0; c < cn; c++)
          if (st.cand_slot[DG_CAND * k + c] == sup) atomicOr(&bm[c][va >> 5], 1u << (va & 31));
      }
      wave_sync();
      uint32_t certifies = 0;
      for (uint32_t c = 0; c < cn; c++) {
        const uint64_t stake = bitmap_stake(bm[c], stakes, n_auth);
        if (stake > quorum_thr) certifies |= 1u << c;
        if (lane == 0 && stake > quorum_thr)
          atomicOr(st.cert + DG_BM * (DG_CAND * k + c) + (author >> 5), 1u << (author & 31));
      }
      if (st.cmask && lane == 0) st.cmask[di * in.gmax + j] = (uint8_t)certifies;  // (this wave's own byte; a commit call reads it)
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_dg_decide(const u64* __restrict__ slots, uint64_t n_slots, DecideIn in, DecideState st,
                                                  const uint64_t* __restrict__ stakes, uint32_t n_auth, uint64_t quorum_thr,
                                                  uint64_t* __restrict__ out, uint64_t* __restrict__ stakes_out,
                                                  u64* __restrict__ ctl) {
  const uint64_t k = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  const uint32_t lane = threadIdx.x & 63;
  if (k >= in.n) return;
  const uint64_t a = in.l_auth[k], r = in.l_round[k], row = in.l_row[k];
  if (row >= in.n) return;
  uint64_t w[8] = {a, r, 0, 0, 0, 0, MV_LEADER_UNDECIDED, 0}, sk[3] = {0, 0, 0};
  bool bad = false;
  if (a < n_auth) {
    const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
    const uint64_t blame = bitmap_stake(st.blame + DG_BM * k, stakes, n_auth);
    uint64_t best_v = 0, best_c = 0, com_v = 0, com_c = 0;
    u64 com_slot = DG_NO_SLOT;
    uint32_t enough = 0;
    for (uint32_t c = 0; c < cn; c++) {
      const uint64_t v = bitmap_stake(st.vote + DG_BM * (DG_CAND * k + c), stakes, n_auth);
      const uint64_t ce = bitmap_stake(st.cert + DG_BM * (DG_CAND * k + c), stakes, n_auth);
      if (v > best_v || (v == best_v && ce > best_c)) best_v = v, best_c = ce;
      if (ce > quorum_thr) enough++, com_v = v, com_c = ce, com_slot = st.cand_slot[DG_CAND * k + c];
    }
    const u64 nlo = ctl[mvk::IX_CTL_DG_NLO];  // max of ~round over the records, 0 without any
    uint64_t status = MV_LEADER_UNDECIDED;
    if (nlo == 0 || r < ~nlo) status = MV_LEADER_UNDECIDED;  // below the lowest retained round
    else if (blame > quorum_thr) status = MV_LEADER_SKIP;
    else if (found > DG_CAND) status = MV_LEADER_OVERFLOW;
    else if (enough == 1) status = MV_LEADER_COMMIT;
    else if (enough > 1) status = MV_LEADER_CONFLICT;
    if (status == MV_LEADER_COMMIT) {
      bad = com_slot >= n_slots;
      if (bad) status = MV_LEADER_UNDECIDED;
      else
        for (int i = 0; i < 6; i++) w[i] = slots[SLOT_WORDS * com_slot + 2 + i];
    }
    w[6] = status, w[7] = found;
    sk[0] = blame;
    if (found <= DG_CAND) sk[1] = enough == 1 ? com_v : best_v, sk[2] = enough == 1 ? com_c : best_c;
  }
  if (lane == 0) {
    for (int i = 0; i < 8; i++) out[8 * row + i] = w[i];
    if (stakes_out)
      for (int i = 0; i < 3; i++) stakes_out[3 * row + i] = sk[i];
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && lane == 0);
}

// ---------------------------------------------------------------- the indirect rule and the committed sequence
// mv_commit_leaders: BaseCommitter::try_indirect_decide (base_committer.rs:294-318) with
// decide_leader_from_anchor (:184-224) over BlockStore::linked_to_round (block_store.rs:306-327),
// and the prefix of UniversalCommitter::try_commit (universal_committer.rs:75-90), on top of the
// direct stages above, whose k_dg_cert also leaves the candidates every decision record certifies
// (DecideState::cmask). The rows stand in non-decreasing round order. The memory model is
// index_dev.h's: lanes of one launch talk only through agent-scope atomic read-modify-writes on single
// words (a job claimed by CAS, min / max on a job's words, OR into a mark bitmap, which is also
// read by an atomic OR of 0 where the same launch writes other bits of the word), nobody waits, and
// what a kernel reads as plain data an earlier launch wrote: the chain step reads fin[] and the out
// rows and writes act[]; only the resolve step, a later launch, writes fin[] and the out rows.
//   k_cm_init     a lane per row: rows the direct rule decided are final; the slot of a COMMIT row's block
//   k_cm_chain    a lane per row that is not final: the first row at least three rounds up that is
//                 not SKIP -- not final yet: wait for a later pass; COMMIT: the anchor, whose walk job
//                 is claimed once and takes the lowest target round; anything else: blocked
//   k_cm_seed     a lane per job: the anchor's record into the job's marks
//   SpanList      once per call: the records of the rounds a level can read, a compaction pass
//   k_cm_reach    one launch per level q some job passes, a wave per record of the span, at work when
//                 its round is q + 1: for every job whose walk passes the level and that marks
//                 it, the includes of key round q in batches of 64 -- with a record: marked; without: the
//                 job is incomplete from q up
//   k_cm_resolve  a wave per row the chain step moved: the marked decision records of round r + 2,
//                 their certificate masks, the incomplete tests, the verdict
//   k_cm_prefix   one wave: the sequence's length
using mvk::CommitState;

__device__ inline bool marked(const uint32_t* marks, uint64_t words, uint64_t id, uint64_t rec) {
  return (marks[id * words + (rec >> 5)] >> (rec & 31)) & 1u;
}

__global__ void __launch_bounds__(WG) k_cm_init(const u64* __restrict__ slots, uint64_t n_slots, DecideIn in, DecideState st,
                                                CommitState cs, const uint64_t* __restrict__ out,
                                                uint64_t* __restrict__ info, u64* __restrict__ ctl) {
  const uint64_t k = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (k < in.n) {
    const uint64_t status = out[8 * k + 6];
    u64 at = DG_NO_SLOT;
    if (status == MV_LEADER_COMMIT) {
      const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
      for (uint32_t c = 0; c < cn; c++) {
        const u64 s = st.cand_slot[DG_CAND * k + c];
        if (s >= n_slots) continue;
        bool eq = true;
        for (int w = 0; w < 6; w++) eq &= slots[SLOT_WORDS * s + 2 + w] == out[8 * k + w];
        if (eq) at = s;
      }
      bad = at == DG_NO_SLOT;
    }
    const bool fin = status != MV_LEADER_UNDECIDED;
    cs.fin[k] = fin;
    cs.act[k] = mvk::CM_ACT_NONE;
    cs.anchor[k] = DG_NONE;
    cs.cslot[k] = at;
    info[4 * k] = fin ? 1 : 0, info[4 * k + 1] = ~0ull, info[4 * k + 2] = 0, info[4 * k + 3] = 0;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_cm_chain(DecideIn in, CommitState cs, const uint64_t* __restrict__ out,
                                                 u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t act = mvk::CM_ACT_NONE;
  if (i < in.n && !cs.fin[i]) {
    const uint64_t r = in.l_round[i];
    act = mvk::CM_ACT_UNDECIDED;
    if (r <= ~0ull - 3) {
      uint64_t lo = i + 1, hi = in.n;  // the first row of round >= r + 3
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (in.l_round[mid] < r + 3) lo = mid + 1;
        else hi = mid;
      }
      for (uint64_t j = lo; j < in.n; j++) {  // bounded by the rows
        if (!cs.fin[j]) {
          act = mvk::CM_ACT_NONE;  // decided by a later pass
          break;
        }
        const uint64_t status = out[8 * j + 6];
        if (status == MV_LEADER_SKIP) continue;
        if (status != MV_LEADER_COMMIT) {
          act = mvk::CM_ACT_BLOCKED;
          break;
        }
        act = mvk::CM_ACT_WALK;
        cs.anchor[i] = (uint32_t)j;
        if (atomicCAS(cs.job_id + j, DG_NONE, mvk::CM_CLAIMED) == DG_NONE) {
          const u64 id = atomicAdd(ctl + mvk::IX_CTL_CM_NJOBS, 1ull);
          if (id < in.n) {
            cs.jobs[id] = (uint32_t)j;
            atomicExch(cs.job_id + j, (uint32_t)id);
          }
        }
        atomicMin((u64*)cs.job_low + j, (u64)(r + 2));
        atomicMax(ctl + mvk::IX_CTL_CM_QHI, (u64)in.l_round[j]);
        atomicMax(ctl + mvk::IX_CTL_CM_NQLO, (u64)~(r + 2));
        break;
      }
    }
  }
  if (i < in.n) cs.act[i] = act;
  wave_count_to(ctl + mvk::IX_CTL_CM_MOVED, act != mvk::CM_ACT_NONE);
}

__global__ void __launch_bounds__(WG) k_cm_seed(DagStore d, uint64_t nb, uint64_t n, CommitState cs, uint64_t njobs,
                                                u64* __restrict__ ctl) {
  const uint64_t id = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (id < njobs) {
    const uint64_t j = cs.jobs[id];
    const u64 s = j < n ? cs.cslot[j] : DG_NO_SLOT;
    const uint32_t rec = s < d.n_slots ? d.map[s] : DG_NONE;
    bad = rec >= nb || (rec >> 5) >= cs.mark_words;
    if (!bad) atomicOr(cs.marks + id * cs.mark_words + (rec >> 5), 1u << (rec & 31));
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// the records of rounds lo..hi, the only ones a level of the call can read, in record order
struct SpanList {
  static constexpr int WEIGHTS = 1;
  DagStore d;
  uint64_t nb, lo, hi;
  uint32_t* span;
  __device__ void weigh(uint64_t rec, uint64_t* in) const { *in = rec < nb && d.round[rec] >= lo && d.round[rec] <= hi; }
  __device__ void place(uint64_t rec, uint64_t in, uint64_t at) const {
    if (in && at < nb) span[at] = (uint32_t)rec;
  }
};

__global__ void __launch_bounds__(WG) k_cm_reach(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                 CommitState cs, uint64_t njobs, uint64_t nspan, uint64_t q,
                                                 u64* __restrict__ ctl) {
  const uint64_t w = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record of the span
  const uint32_t lane = threadIdx.x & 63;
  if (w >= nspan) return;
  const uint64_t rec = cs.span[w];
  if (rec >= nb) {
    wave_count_to(ctl + mvk::IX_CTL_ERR, lane == 0);
    return;
  }
  if (d.round[rec] != q + 1 || (rec >> 5) >= cs.mark_words) return;
  const uint64_t base = d.ibase[rec];
  const uint32_t kc = d.kc[rec];
  bool bad = base > d.cap_i || kc > d.cap_i - base;
  if (!bad) {
    for (uint64_t id = 0; id < njobs; id++) {  // bounded by the jobs the host read back
      const uint64_t j = cs.jobs[id];
      if (j >= in.n) {
        bad = true;
        continue;
      }
      if (in.l_round[j] < q + 1 || cs.job_low[j] > q) continue;  // the job's walk does not pass this level
      // (this launch sets bits of round-q records in the same words: read through an atomic)
      uint32_t word = 0;
      if (lane == 0) word = atomicOr(cs.marks + id * cs.mark_words + (rec >> 5), 0u);
      word = (uint32_t)__shfl((int)word, 0);
      if (!((word >> (rec & 31)) & 1u)) continue;
      bool miss = false;
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
        const uint32_t x = q0 + lane;
        if (x >= kc) continue;
        const u64 s = d.inc[base + x];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        if (slots[SLOT_WORDS * s + 3] != q) continue;  // a weak link leads nowhere (block_store.rs:312-321)
        const uint32_t v = d.map[s];
        if (v == DG_NONE) miss = true;
        else if (v >= nb || (v >> 5) >= cs.mark_words) bad = true;
        else atomicOr(cs.marks + id * cs.mark_words + (v >> 5), 1u << (v & 31));
      }
      if (__ballot(miss) != 0 && lane == 0) atomicMax((u64*)cs.job_miss + j, (u64)(q + 1));
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_cm_resolve(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                   DecideState st, CommitState cs, uint64_t nvote, uint64_t ndec,
                                                   uint64_t njobs, uint64_t* __restrict__ out, uint64_t* __restrict__ info,
                                                   u64* __restrict__ ctl) {
  const uint64_t i = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  const uint32_t lane = threadIdx.x & 63;
  if (i >= in.n) return;
  const uint32_t act = cs.act[i];
  if (act == mvk::CM_ACT_NONE) return;
  if (act != mvk::CM_ACT_WALK) {
    if (lane == 0) {
      cs.fin[i] = 1;
      info[4 * i + 2] = act == mvk::CM_ACT_BLOCKED ? 2 : 0;
    }
    return;
  }
  const uint64_t r = in.l_round[i], j = cs.anchor[i];
  const uint64_t id = j < in.n ? cs.job_id[j] : DG_NONE;
  uint64_t g = 0;
  bool bad = id >= njobs || !leader_group(in, r, &g) || i < in.g_start[g] || i - in.g_start[g] >= in.gmax;
  uint32_t mask = 0;
  uint64_t count = 0;
  bool incomplete = false;
  if (!bad) {
    const uint64_t jrow = i - in.g_start[g];
    for (uint64_t di = lane; di < ndec; di += 64) {  // bounded by the decision records the host read back
      const uint32_t rec = st.dlist[di];
      if (rec >= nb || (rec >> 5) >= cs.mark_words) {
        bad = true;
        continue;
      }
      if (d.round[rec] != r + 2 || !marked(cs.marks, cs.mark_words, id, rec)) continue;
      count++;
      mask |= st.cmask[di * in.gmax + jrow];
      const uint64_t base = d.ibase[rec];
      const uint32_t kc = d.kc[rec];
      if (base > d.cap_i || kc > d.cap_i - base) {
        bad = true;
        continue;
      }
      for (uint32_t x = 0; x < kc; x++) {  // a voting block without a record, or one whose support has none
        const u64 s = d.inc[base + x];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        if (slots[SLOT_WORDS * s + 3] != r + 1) continue;
        const uint32_t v = d.map[s];
        if (v == DG_NONE) {
          incomplete = true;
          continue;
        }
        const uint32_t vp = v < nb ? st.vpos[v] : DG_NONE;
        if (vp >= nvote) continue;
        const u64 sup = st.sup[(uint64_t)vp * in.gmax + jrow];
        if (sup == DG_NO_SLOT) continue;
        if (sup >= d.n_slots) bad = true;
        else if (d.map[sup] == DG_NONE) incomplete = true;
      }
    }
  }
  for (int w = 32; w; w >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, w);
  count = wave_sum64(count);
  incomplete = __ballot(incomplete) != 0;
  bad = __ballot(bad) != 0;
  if (lane == 0 && !bad) {
    const u64 nlo = ctl[mvk::IX_CTL_DG_NLO];  // (written by a connect call or a prune, earlier launches)
    incomplete = incomplete || nlo == 0 || r < ~nlo || cs.job_miss[j] >= r + 3;
    const uint32_t found = st.cand_n[i], cn = found < DG_CAND ? found : DG_CAND;
    mask &= (1u << cn) - 1;
    const int ncert = __popc(mask);
    uint64_t status = MV_LEADER_UNDECIDED, kind = 2;
    u64 com = DG_NO_SLOT;
    if (found > DG_CAND) status = MV_LEADER_OVERFLOW;  // (defensive: the direct rule already ended such a row)
    else if (ncert == 1) status = MV_LEADER_COMMIT, com = st.cand_slot[DG_CAND * i + (__ffs((int)mask) - 1)];
    else if (ncert > 1) status = MV_LEADER_CONFLICT;
    else if (incomplete) kind = 0;
    else status = MV_LEADER_SKIP;
    if (status == MV_LEADER_COMMIT) {
      if (com >= d.n_slots) bad = true;
      else
        for (int w = 0; w < 6; w++) out[8 * i + w] = slots[SLOT_WORDS * com + 2 + w];
    }
    if (!bad) {
      out[8 * i + 6] = status;
      cs.cslot[i] = com;
      info[4 * i] = kind, info[4 * i + 1] = j, info[4 * i + 2] = incomplete ? 1 : 0, info[4 * i + 3] = count;
    }
  }
  if (lane == 0) cs.fin[i] = 1;
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && lane == 0);
}

__global__ void __launch_bounds__(64) k_cm_prefix(DecideIn in, const uint64_t* __restrict__ out, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x;
  uint64_t first = in.n, zero = 0;
  for (uint64_t i = lane; i < in.n; i += 64) {  // bounded by the rows
    if (in.l_round[i] == 0) {
      zero++;
      continue;
    }
    const uint64_t status = out[8 * i + 6];
    if (status != MV_LEADER_COMMIT && status != MV_LEADER_SKIP && i < first) first = i;
  }
  for (int w = 32; w; w >>= 1) {
    const uint64_t o = shfl64(first, lane ^ w);
    first = o < first ? o : first;
  }
  zero = wave_sum64(zero);
  if (lane == 0) atomicExch(ctl + mvk::IX_CTL_CM_NSEQ, (u64)(first >= zero ? first - zero : 0));
}

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_decide_pick(const DagStore& d, uint64_t nb, const DecideIn& in, const DecideState& st, uint64_t* wg,
                              uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  compact_pass(PickRoles{d, nb, in, st}, nb, wg_scan_of(wg, nb), ctl + IX_CTL_DG_NVOTE, ctl + IX_CTL_DG_NDEC, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_decide_rule(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                              const DecideState& st, uint64_t nvote, uint64_t ndec, const uint64_t* stakes,
                              uint32_t n_auth, uint64_t quorum_thr, uint64_t* out, uint64_t* stakes_out, uint64_t* ctl,
                              hipStream_t s) {
  if (n_auth > DG_MAX_AUTH) return hipErrorInvalidValue;
  const dim3 b(WG);
  if (nvote) {
    hipError_t e = hipMemsetAsync(st.sup, 0xff, 8 * nvote * in.gmax, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dg_vote, dim3(grid_of(64 * nvote * in.gmax)), b, 0, s, (const u64*)t.slots, d, nb, in, st, nvote,
                       (u64*)ctl);
  }
  if (ndec && nvote)
    hipLaunchKernelGGL(k_dg_cert, dim3(grid_of(64 * ndec * in.gmax)), b, 0, s, d, nb, in, st, nvote, ndec, stakes, n_auth,
                       quorum_thr, (u64*)ctl);
  hipLaunchKernelGGL(k_dg_decide, dim3(grid_of(64 * in.n)), b, 0, s, (const u64*)t.slots, d.n_slots, in, st, stakes, n_auth,
                     quorum_thr, out, stakes_out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_init(const IndexTable& t, const DecideIn& in, const DecideState& st, const CommitState& cs,
                              const uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_init, dim3(grid_of(in.n)), dim3(WG), 0, s, (const u64*)t.slots, t.mask + 1, in, st, cs, out, info,
                     (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_chain(const DecideIn& in, const CommitState& cs, const uint64_t* out, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_chain, dim3(grid_of(in.n)), dim3(WG), 0, s, in, cs, out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_span(const DagStore& d, uint64_t nb, uint64_t lo, uint64_t hi, uint32_t* span, uint64_t* wg,
                              uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  compact_pass(SpanList{d, nb, lo, hi, span}, nb, wg_scan_of(wg, nb), ctl + IX_CTL_CM_NSPAN, nullptr, nullptr, s);
  return hipGetLastError();
}

hipError_t launch_commit_reach(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                               const CommitState& cs, uint64_t njobs, uint64_t nspan, const uint64_t* levels,
                               uint64_t n_levels, uint64_t* ctl, hipStream_t s) {
  if (njobs == 0 || nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cm_seed, dim3(grid_of(njobs)), dim3(WG), 0, s, d, nb, in.n, cs, njobs, (u64*)ctl);
  if (nspan == 0) return hipGetLastError();
  for (uint64_t k = 0; k < n_levels; k++)  // downwards
    hipLaunchKernelGGL(k_cm_reach, dim3(grid_of(64 * nspan)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, in, cs, njobs, nspan,
                       levels[k], (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_resolve(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                                 const DecideState& st, const CommitState& cs, uint64_t nvote, uint64_t ndec, uint64_t njobs,
                                 uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_resolve, dim3(grid_of(64 * in.n)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, in, st, cs, nvote,
                     ndec, njobs, out, info, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_prefix(const DecideIn& in, const uint64_t* out, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_prefix, dim3(1), dim3(64), 0, s, in, out, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
