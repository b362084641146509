// The linearizer over the DAG store (dag_store.hip). mv_linearize: Linearizer::handle_commit with
// collect_sub_dag (consensus/linearizer.rs:125-166, :58-105); the rule, level by level, is the
// header's. The reference marks a block when it is pushed, so a block belongs to the includer that
// is popped first: of all pairs (member x, include number j) that name it, the least (path(x), j),
// where path(b) = path(x) ++ (0xffff - j). All leaders of a call go through one top-down sweep:
// cidx(b), the sequence number of the first leader that reaches b, is the least cidx of its
// includers, so the least key (cidx(x), path(x), j) decides leader and parent at once.
// The key is LN_KEY_WORDS words -- 16 bits of cidx, the includer's 16 path components, 16 bits of j --
// and its minimum is taken word by word, one launch per word: a lane goes on to word w only while its
// words before w equal the minima the earlier launches left. This is exact and needs no rank of the
// nodes (a scalar that is monotone in the path would need a sort per level to stay so).
// The memory model is index_dev.h's: inside one launch lanes talk only through agent-scope atomic
// read-modify-writes on single words (min on a key word, add on a counter, max on a status), nobody
// waits, and what a kernel reads as plain data an earlier launch wrote. Every slot, record, node,
// bucket and edge number is checked against its array before it is an address; a failed check counts
// into the error word and is not followed. Every loop is bounded by a count read under such a check.
//   k_ln_roots   a lane per leader: its slot by a probe of the table; no entry or no record:
//                INCOMPLETE, marked: COMMITTED; else its root key (cidx, empty path) into word 0
//   k_ln_edges   a wave per record of round <= the highest leader round: its includes, bucketed by the
//                included reference's round (bucket 0: the rounds below the store's lowest) -- the
//                counts (one add per bucket and batch of 64), and after the host's scan of them the
//                edges and, per record, the lowest round of an include not marked before the call
//   k_ln_pick    one launch per key word and level, a lane per edge that ends in the level: min
//   k_ln_take    a lane per edge of the level and per leader: the edge whose whole key is the minimum
//                (there is one: (x, j) is its own) makes the node -- cidx, path, its number among the
//                leader's nodes -- or the leader's failure; a leader whose slot holds its root key makes
//                its root, one whose slot holds a lower key is COMMITTED; every new node lowers the
//                call's lowest reachable round, which the host reads to end the sweep
//   k_ln_rows    one wave: statuses, the prefix rule, first rows, counts, heights
//   k_ln_out     a lane per node of the OK prefix: its place among the nodes of its level and leader by
//                counting those below it, behind the leader's nodes of lower levels; the row, the mark
//   k_ln_mark    mv_linearize_mark: the marks of an insert's items
//   k_ln_carry   after a rebuild: a marked slot of the old table marks its key's slot in the new one
#include "index_dev.h"

namespace mv::ix {

using mvk::LinEdge;
using mvk::LinState;
constexpr int LN_KW = mvk::LN_KEY_WORDS, LN_PW = mvk::LN_PATH_WORDS;

__device__ inline void lin_fail(const LinState& ls, uint32_t cidx, uint32_t status) {
  if (cidx < ls.n) atomicMax(ls.fail + cidx, status);
}
// word w of the key (cidx, path words p, j)
__device__ inline u64 key_word(uint32_t cidx, const u64* p, uint32_t j, int w) {
  if (w == 0) return ((u64)cidx << 48) | (p[0] >> 16);
  if (w < LN_PW) return ((p[w - 1] & 0xffffull) << 48) | (p[w] >> 16);
  return ((p[LN_PW - 1] & 0xffffull) << 48) | ((u64)j << 32);
}

__global__ void __launch_bounds__(WG) k_ln_roots(IndexTable t, DagStore d, uint64_t nb, LinState ls, u64* __restrict__ ctl) {
  const uint64_t k = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (k < ls.n) {
    uint64_t key[6];
    for (int w = 0; w < 6; w++) key[w] = ls.leaders[6 * k + w];
    uint32_t probe;  // (not reported: this call's probes never were)
    u64 s = find_slot(t, key, &probe, &bad);
    uint32_t fail = 0;
    if (s >= d.n_slots) {
      fail = MV_LINEAR_INCOMPLETE;
    } else if (ls.mark[s]) {  // (set by an earlier call)
      fail = MV_LINEAR_COMMITTED;
    } else {
      const uint32_t rec = d.map[s];
      if (rec == DG_NONE) fail = MV_LINEAR_INCOMPLETE;
      else if (rec >= nb) bad = true;
    }
    if (fail || bad) s = DG_NO_SLOT;
    ls.root_slot[k] = s;
    ls.fail[k] = fail;
    ls.total[k] = 0;
    if (s != DG_NO_SLOT) atomicMin((u64*)ls.best + LN_KW * s, (u64)k << 48);
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_ln_edges(const u64* __restrict__ slots, DagStore d, uint64_t nb, LinState ls, bool fill,
                                                 u64* __restrict__ ctl) {
  const uint64_t rec = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  const uint32_t lane = threadIdx.x & 63;
  if (rec >= nb) return;
  const uint64_t rd = d.round[rec];
  if (rd > ls.hi) return;
  const uint64_t base = d.ibase[rec];
  const uint32_t kc = d.kc[rec];
  bool bad = base > d.cap_i || kc > d.cap_i - base;
  u64 low = ~0ull;
  if (!bad) {
    for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
      const uint32_t q = q0 + lane;
      u64 s = DG_NO_SLOT, tr = 0;
      uint64_t bk = 0;
      bool want = false;
      if (q < kc) {
        s = d.inc[base + q];
        if (s >= d.n_slots) {
          bad = true;
        } else {
          tr = slots[SLOT_WORDS * s + 3];
          // (threshold_clock.rs:18-22: an include lies below its block; not followed otherwise)
          if (tr < rd) {
            if (tr < low && !ls.mark[s]) low = tr;
            bk = tr >= ls.lo ? tr - ls.lo + 1 : 0;
            want = bk < ls.nbk;
            bad = bad || !want;
          }
        }
      }
      // one add per bucket and batch, not per include: the includes of a block mostly end in one round,
      // and an add per include on the same word serialises (12 ms of a call at 2.2 M includes)
      uint32_t at = 0;
      u64 todo = __ballot(want);
      while (todo) {  // every turn retires at least its first lane: 64 turns at most
        const int head = __ffsll((long long)todo) - 1;
        const uint64_t hbk = shfl64(bk, head);  // (below nbk: the head lane wants)
        const u64 same = __ballot(want && bk == hbk);
        uint32_t start = 0;
        if ((int)lane == head) start = atomicAdd(ls.bk_count + hbk, (uint32_t)__popcll(same));
        start = (uint32_t)__shfl((int)start, head);
        if (want && bk == hbk) at = start + (uint32_t)__popcll(same & ((1ull << lane) - 1));
        todo &= ~same;
      }
      if (!fill || !want) continue;
      const uint64_t e = ls.bk_off[bk] + at;
      if (e >= ls.bk_off[bk + 1] || e >= ls.n_edges) {
        bad = true;
        continue;
      }
      ls.edges[e] = LinEdge{(uint32_t)rec, q, s};
    }
  }
  if (fill) {  // (the wave is whole here: every lane left the loop)
    for (int dd = 32; dd; dd >>= 1) {
      const u64 o = shfl64(low, (int)(lane ^ dd));
      low = o < low ? o : low;
    }
    if (lane == 0) ls.rec_low[rec] = low;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// An edge at work: its includer is a node, the included reference is not marked. Its key words.
__device__ inline bool edge_key(const LinState& ls, uint64_t n_slots, uint64_t nb, uint64_t nnodes, const LinEdge& e, u64 kw[LN_KW],
                                uint32_t* node, bool* bad) {
  if (e.rec >= nb || e.slot >= n_slots) {
    *bad = true;
    return false;
  }
  const uint32_t x = ls.node_of_rec[e.rec];  // (a take step of a level above, an earlier launch)
  if (x == DG_NONE) return false;
  if (x >= nnodes || x >= ls.node_cap) {
    *bad = true;
    return false;
  }
  if (ls.mark[e.slot]) return false;
  u64 p[LN_PW];
  for (int w = 0; w < LN_PW; w++) p[w] = ls.n_path[LN_PW * (uint64_t)x + w];
  const uint32_t cidx = ls.n_cidx[x], j = e.j < mvk::LN_MAX_J ? e.j : mvk::LN_MAX_J;
  for (int w = 0; w < LN_KW; w++) kw[w] = key_word(cidx, p, j, w);
  *node = x;
  return true;
}

// nnodes: the nodes made before this level (the host cannot know it: read from the counter, which no pick launch writes)
__global__ void __launch_bounds__(WG) k_ln_pick(DagStore d, uint64_t nb, LinState ls, uint64_t level, uint64_t e0, uint64_t ne,
                                                int word, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const u64 nnodes = ls.lctl[mvk::LN_CTL_NNODES];  // (written by take steps, earlier launches)
  if (i == 0 && word == 0 && level < ls.n_levels) ls.lvl_start[level] = nnodes;
  bool bad = false;
  if (i < ne && e0 + i < ls.n_edges) {
    const LinEdge e = ls.edges[e0 + i];
    u64 kw[LN_KW];
    uint32_t x;
    if (edge_key(ls, d.n_slots, nb, nnodes, e, kw, &x, &bad)) {
      u64* best = (u64*)ls.best + LN_KW * e.slot;
      bool tied = true;
      for (int w = 0; w < word; w++) tied = tied && best[w] == kw[w];  // (the launches of the words before)
      if (tied) atomicMin(best + word, kw[word]);
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__device__ inline uint32_t new_node(const LinState& ls, u64 slot, u64 round, uint32_t cidx, uint32_t depth, const u64* p,
                                    uint64_t level, bool* bad) {
  const u64 id = atomicAdd((u64*)ls.lctl + mvk::LN_CTL_NNODES, 1ull);
  if (id >= ls.node_cap || cidx >= ls.n) {
    *bad = true;
    return DG_NONE;
  }
  ls.n_slot[id] = slot, ls.n_round[id] = round, ls.n_cidx[id] = cidx, ls.n_depth[id] = depth, ls.n_lvl[id] = (uint32_t)level;
  for (int w = 0; w < LN_PW; w++) ls.n_path[LN_PW * id + w] = p[w];
  ls.n_t[id] = atomicAdd(ls.total + cidx, 1u);
  return (uint32_t)id;
}
// a record became a node: its unmarked includes may give the levels down to rec_low work
__device__ inline void node_reaches(const LinState& ls, uint32_t rec) {
  const u64 low = ls.rec_low[rec];  // (the edge walk, an earlier launch)
  if (low != ~0ull) atomicMin((u64*)ls.lctl + mvk::LN_CTL_LO, low);
}

__global__ void __launch_bounds__(WG) k_ln_take(const u64* __restrict__ slots, DagStore d, uint64_t nb, LinState ls, uint64_t level,
                                                uint64_t round, uint64_t e0, uint64_t ne, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (level >= ls.n_levels) return;
  const u64 nnodes = ls.lvl_start[level];  // (this level's first pick launch)
  if (i < ne && e0 + i < ls.n_edges) {
    const LinEdge e = ls.edges[e0 + i];
    u64 kw[LN_KW];
    uint32_t x;
    if (edge_key(ls, d.n_slots, nb, nnodes, e, kw, &x, &bad)) {
      const u64* best = (const u64*)ls.best + LN_KW * e.slot;
      bool won = true;
      for (int w = 0; w < LN_KW; w++) won = won && best[w] == kw[w];
      if (won) {
        const uint32_t cidx = ls.n_cidx[x], depth = ls.n_depth[x];
        const uint32_t rec = d.map[e.slot];
        const u64 tr = slots[SLOT_WORDS * e.slot + 3];
        if (depth >= mvk::LN_MAX_DEPTH || e.j >= mvk::LN_MAX_J) {
          lin_fail(ls, cidx, MV_LINEAR_OVERFLOW);
        } else if (rec == DG_NONE && tr != 0) {
          lin_fail(ls, cidx, MV_LINEAR_INCOMPLETE);
        } else if (rec != DG_NONE && rec >= nb) {
          bad = true;
        } else {
          u64 p[LN_PW];
          for (int w = 0; w < LN_PW; w++) p[w] = ls.n_path[LN_PW * (uint64_t)x + w];
          p[depth / 4] |= (u64)(0xffffu - e.j) << (48 - 16 * (depth % 4));
          const uint32_t id = new_node(ls, e.slot, tr, cidx, depth + 1, p, level, &bad);
          if (id != DG_NONE && rec != DG_NONE) {
            ls.node_of_rec[rec] = id;  // (one winner per slot, one slot per record)
            node_reaches(ls, rec);
          }
        }
      }
    }
  } else if (i >= ne && i - ne < ls.n) {
    const uint64_t k = i - ne;
    const u64 s = ls.root_slot[k];
    if (s < d.n_slots && ls.leaders[6 * k + 1] == round) {
      const u64 w0 = ls.best[LN_KW * s];
      if (w0 == ((u64)k << 48)) {
        const uint32_t rec = d.map[s];
        if (rec >= nb) {
          bad = true;
        } else {
          const u64 p[LN_PW] = {0, 0, 0, 0};
          const uint32_t id = new_node(ls, s, round, (uint32_t)k, 0, p, level, &bad);
          if (id != DG_NONE) {
            ls.node_of_rec[rec] = id;
            node_reaches(ls, rec);
          }
        }
      } else {
        lin_fail(ls, (uint32_t)k, MV_LINEAR_COMMITTED);  // an earlier leader of the call reached it, or stands on it
      }
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(64) k_ln_rows(LinState ls, uint64_t height0, uint64_t cap, uint64_t* __restrict__ sub) {
  const uint32_t lane = threadIdx.x;
  uint64_t rows = 0, nok = 0;
  bool stopped = false;
  for (uint64_t k0 = 0; k0 < ls.n; k0 += 64) {  // bounded by the leaders
    const uint64_t k = k0 + lane;
    const uint64_t cnt = k < ls.n ? ls.total[k] : 0;
    uint64_t inc = cnt;
    for (int dd = 1; dd < 64; dd <<= 1) {
      const uint64_t o = shfl64(inc, (int)lane - dd < 0 ? 0 : (int)lane - dd);
      if (lane >= (uint32_t)dd) inc += o;
    }
    const uint64_t first = rows + inc - cnt;
    uint32_t status = k < ls.n ? ls.fail[k] : 0;
    if (k < ls.n && !status && (first > cap || cnt > cap - first)) status = MV_LINEAR_OVERFLOW;
    const u64 m = stopped ? ~0ull : __ballot(k < ls.n && status != MV_LINEAR_OK);
    const uint32_t f = m ? (uint32_t)__ffsll((long long)m) - 1 : 64;  // the first lane that is not OK
    const uint64_t ok_rows = f < 64 ? shfl64(first, (int)f) : rows + shfl64(inc, 63);
    if (k < ls.n) {
      const bool ok = lane < f;
      if (!ok && (stopped || lane > f)) status = MV_LINEAR_STOPPED;
      sub[4 * k] = status;
      sub[4 * k + 1] = ok ? first : ok_rows;
      sub[4 * k + 2] = ok ? cnt : 0;
      sub[4 * k + 3] = ok ? height0 + k + 1 : 0;
      ls.first[k] = first;
    }
    if (!stopped) {
      const uint64_t left = ls.n - k0;
      nok += f < 64 ? f : (left < 64 ? left : 64);
      rows = ok_rows;
    }
    if (m) stopped = true;
  }
  if (lane == 0) {
    atomicExch((u64*)ls.lctl + mvk::LN_CTL_NOK, (u64)nok);
    atomicExch((u64*)ls.lctl + mvk::LN_CTL_NROWS, (u64)rows);
    if (ls.n_levels) ls.lvl_start[ls.n_levels] = ls.lctl[mvk::LN_CTL_NNODES];
  }
}

// (round, path) of node a below that of node b
__device__ inline bool node_below(const LinState& ls, uint64_t a, uint64_t b) {
  if (ls.n_round[a] != ls.n_round[b]) return ls.n_round[a] < ls.n_round[b];
  for (int w = 0; w < LN_PW; w++) {
    const u64 x = ls.n_path[LN_PW * a + w], y = ls.n_path[LN_PW * b + w];
    if (x != y) return x < y;
  }
  return false;
}

__global__ void __launch_bounds__(WG) k_ln_out(const u64* __restrict__ slots, uint64_t n_slots, LinState ls, uint64_t cap,
                                               uint64_t* __restrict__ blocks, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const u64 nnodes = ls.lctl[mvk::LN_CTL_NNODES], nok = ls.lctl[mvk::LN_CTL_NOK], nrows = ls.lctl[mvk::LN_CTL_NROWS];
  bool bad = false, fresh = false;
  if (i < nnodes && i < ls.node_cap) {
    const uint32_t cidx = ls.n_cidx[i], lvl = ls.n_lvl[i];
    if (cidx < nok && cidx < ls.n) {
      bad = lvl >= ls.n_levels;
      const uint64_t a = bad ? 0 : ls.lvl_start[lvl], b = bad ? 0 : ls.lvl_start[lvl + 1];
      bad = bad || a > i || b <= i || b > nnodes || b > ls.node_cap;
      if (!bad) {
        // the leader's nodes of this level: how many, how many below this one, the least take number
        uint64_t group = 0, below = 0, t0 = ls.n_t[i];
        for (uint64_t o = a; o < b; o++) {  // bounded by the level's nodes
          if (ls.n_cidx[o] != cidx) continue;
          group++;
          below += node_below(ls, o, i);
          t0 = ls.n_t[o] < t0 ? ls.n_t[o] : t0;
        }
        // the levels run downwards: the leader's nodes of the levels behind this one come first
        const uint64_t total = ls.total[cidx], s = ls.n_slot[i];
        bad = t0 + group > total || s >= n_slots;
        const uint64_t row = bad ? 0 : ls.first[cidx] + (total - t0 - group) + below;
        bad = bad || row >= nrows || row >= cap;
        if (!bad) {
          for (int w = 0; w < 6; w++) blocks[6 * row + w] = slots[SLOT_WORDS * s + 2 + w];
          fresh = atomicExch(ls.mark + s, 1u) == 0;
        }
      }
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
  wave_count_to((u64*)ls.lctl + mvk::LN_CTL_NEWMARK, fresh);
}

__global__ void __launch_bounds__(WG) k_ln_mark(const u64* __restrict__ item, uint64_t n, uint32_t* __restrict__ mark,
                                                uint64_t n_slots, u64* __restrict__ lctl, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false, fresh = false;
  if (i < n) {
    const u64 it = item[i];
    const uint64_t s = it & SLOT_MASK;
    bad = !item_has_slot(it) || s >= n_slots;
    if (!bad) fresh = atomicExch(mark + s, 1u) == 0;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
  wave_count_to(lctl + mvk::LN_CTL_NEWMARK, fresh);
}

__global__ void __launch_bounds__(WG) k_ln_carry(const u64* __restrict__ old, uint64_t n_old, const uint32_t* __restrict__ old_mark,
                                                 IndexTable t, uint32_t* __restrict__ mark, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (i < n_old && old_mark[i] && old[SLOT_WORDS * i] != 0) {
    uint64_t k[6];
    for (int w = 0; w < 6; w++) k[w] = old[SLOT_WORDS * i + 2 + w];
    uint32_t probe;
    const u64 s = find_slot(t, k, &probe, &bad);
    if (s > t.mask) bad = true;
    else atomicExch(mark + s, 1u);
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_linear_roots(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, uint64_t* ctl,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_ln_roots, dim3(grid_of(ls.n)), dim3(WG), 0, s, t, d, nb, ls, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_linear_edges(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, bool fill,
                               uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ln_edges, dim3(grid_of(64 * nb)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, ls, fill, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_linear_level(const IndexTable& t, const DagStore& d, uint64_t nb, const LinState& ls, uint64_t level,
                               uint64_t round, uint64_t e0, uint64_t ne, uint64_t* ctl, hipStream_t s) {
  const dim3 g(grid_of(ne ? ne : 1)), b(WG);
  for (int w = 0; w < LN_KEY_WORDS; w++) {
    hipLaunchKernelGGL(k_ln_pick, g, b, 0, s, d, nb, ls, level, e0, ne, w, (u64*)ctl);
    if (ne == 0) break;  // (the level's first pick launch also notes where its nodes start)
  }
  hipLaunchKernelGGL(k_ln_take, dim3(grid_of(ne + ls.n)), b, 0, s, (const u64*)t.slots, d, nb, ls, level, round, e0, ne, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_linear_output(const IndexTable& t, const LinState& ls, uint64_t height0, uint64_t cap, uint64_t* sub,
                                uint64_t* blocks, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_ln_rows, dim3(1), dim3(64), 0, s, ls, height0, cap, sub);
  if (ls.node_cap && t.slots)
    hipLaunchKernelGGL(k_ln_out, dim3(grid_of(ls.node_cap)), dim3(WG), 0, s, (const u64*)t.slots, t.mask + 1, ls, cap, blocks,
                       (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_linear_mark(const uint64_t* item, uint64_t n, uint32_t* mark, uint64_t n_slots, uint64_t* lctl,
                              uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ln_mark, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)item, n, mark, n_slots, (u64*)lctl, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_linear_carry(const uint64_t* old_slots, uint64_t n_old, const uint32_t* old_mark, const IndexTable& t,
                               uint32_t* mark, uint64_t* ctl, hipStream_t s) {
  if (n_old == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ln_carry, dim3(grid_of(n_old)), dim3(WG), 0, s, (const u64*)old_slots, n_old, old_mark, t, mark,
                     (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
