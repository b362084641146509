// Transaction votes on the device (include/mysti_verify.h: mv_aggregate_votes): what
// TransactionAggregator::process_block (committee.rs:263-482) does with the Share, Vote and VoteRange
// statements of the blocks BlockHandler::handle_blocks receives (block_handler.rs:146-190), restated
// per cell. The store's layout and a call's arrays: kernels.h (VoteStore, VoteCall).
//
// One call:
//   k_vt_scan      a lane per block: block_walk (bincode_walk.h, NoSink) decides whether it parses,
//                  a statement walk counts its Share runs and vote events
//   (host)         the event total sizes the lists; the sharing blocks' references go into the
//                  store's table by index.hip's insert rounds (launch_index_round on this table)
//   k_vt_rows      a row and a run of zeroed cells per new reference
//   k_vt_emit      the second walk writes the events, each with its row (a read-only probe) and
//                  its range clipped to the row's cells; what lies outside is unknown at once
//   per segment    k_vt_count / scan / k_vt_scatter / k_vt_order group the events by row in id
//                  order; k_vt_apply runs a wave per row through its events one after another, its
//                  lanes spread over the offsets of the event's range -- the reference's order per
//                  cell, no cell written by two lanes; a scan of the events' certified counts; and
//                  k_vt_certs writes each event's rows in ascending offset.
//   k_vt_blockout  the per-block counts from the events'
// A cell certified in a call holds the mark of its event until k_vt_certs has written its row, so
// it can be certified once per segment: a segment ends ahead of every block that registers into a
// row that was there before it (the same block processed again), which is the only way a cell is
// registered after it was certified. Most calls are one segment.
//
// Memory safety: every row, cell, event and list number is held against its array before it becomes
// an address; a failure adds to ctl[VT_CTL_ERR] (the host returns MV_E_HIP) and skips the access.
// Ranges are clipped to the row's cell count, which is a parsed block's statement count: no loop
// is sized by a statement's own numbers.
#include "index_dev.h"

#include "bincode_walk.h"
#include "votes_walk.h"

namespace mv::ix {

using mvk::VoteCall;
using mvk::VoteSeg;
using mvk::VoteStore;

namespace {

constexpr uint64_t VT_MAX_RANGE = 1ull << 20;  // types.rs:447-453
constexpr uint32_t VT_NO_ROW = 0xffffffffu;

__device__ inline void vt_err(u64* ctl) { atomicAdd(ctl + mvk::VT_CTL_ERR, 1ull); }

// what a Vote(Accept) or VoteRange comes to: 0 nothing (an empty range), 1 an event, else its flag bit (2 or 4)
__device__ inline uint32_t vote_kind(uint64_t lo) { return lo == ~0ull ? MV_VOTES_FLAG_OFFSET : 1u; }
__device__ inline uint32_t range_kind(uint64_t s0, uint64_t s1) {
  if (s1 < s0 || s1 - s0 >= VT_MAX_RANGE) return MV_VOTES_FLAG_RANGE;
  return s0 == s1 ? 0u : 1u;
}

struct ScanF {
  bool votes;
  uint64_t last_share = ~0ull - 1;
  uint32_t nreg = 0, nvote = 0, flags = 0;
  __device__ void share(uint64_t k) {
    if (last_share + 1 != k) nreg++;
    last_share = k;
  }
  __device__ void tally(uint32_t kind) {
    if (!votes) return;
    if (kind == 1) nvote++;
    else flags |= kind;
  }
  __device__ void vote(uint64_t, const uint64_t*, uint64_t lo) { tally(vote_kind(lo)); }
  __device__ void reject(uint64_t) {
    if (votes) flags |= MV_VOTES_FLAG_REJECT;  // (not through tally: the bit's value is the event's)
  }
  __device__ void range(uint64_t, const uint64_t*, uint64_t s0, uint64_t s1) { tally(range_kind(s0, s1)); }
};

__device__ inline bool block_span_ok(const VoteCall& c, uint64_t i) {
  const uint64_t o = c.off[i], l = c.len[i];
  return o <= c.buf_bytes && l <= c.buf_bytes - o;
}

__global__ void __launch_bounds__(WG) k_vt_scan(VoteCall c, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool sharing = false;
  uint64_t cells = 0;
  if (i < c.n) {
    uint32_t st = MV_VOTES_PARSE_ERROR, author = 0, nst = 0;
    ScanF f;
    f.votes = !(c.flags & MV_VOTES_REGISTER_ONLY);
    uint64_t key[6] = {0, 0, 0, 0, 0, 0};
    if (block_span_ok(c, i)) {
      BcReader r{c.buf + c.off[i], c.len[i], 0, true};
      NoSink sink;
      IncCount vis;
      if (block_walk(r, sink, vis)) {
        // (the walk parsed: the own reference and vis.n_inc includes lie inside the block)
        BcReader q{r.p, r.len, br::INC_OFF + br::REF_BYTES * vis.n_inc, true};
        uint64_t count = 0;
        if (walk_statements(q, f, &count) && count < (1ull << 31)) {
          ref_key(ld64(r.p), ld64(r.p + 8), r.p + 24, key);
          nst = (uint32_t)count;
          if (key[0] < c.n_auth) {
            st = MV_VOTES_OK;
            author = (uint32_t)key[0];
          } else {
            st = MV_VOTES_UNKNOWN_AUTHOR;
          }
        }
      }
    }
    const bool ok = st == MV_VOTES_OK;
    sharing = ok && f.nreg != 0;
    cells = sharing ? nst : 0;
    c.status[i] = (uint8_t)st;
#pragma unroll
    for (int w = 0; w < 6; w++) c.key[6 * i + w] = key[w];
    c.keyoff[i] = sharing ? 48 * i : mvk::IX_NO_SRC;
    c.author[i] = author;
    c.n_st[i] = nst;
    c.nreg[i] = ok ? f.nreg : 0;
    c.nev[i] = ok ? f.nreg + f.nvote : 0;
    c.bflags[i] = ok ? f.flags : 0;
    c.unk[i] = 0;
    c.brk[i] = 0;
  }
  wave_count_to(ctl + mvk::VT_CTL_NSHARE, sharing);
  cells = wave_sum64(cells);
  if ((threadIdx.x & 63) == 0 && cells) atomicAdd(ctl + mvk::VT_CTL_NEWCELLS, (u64)cells);
}

// ---------------------------------------------------------------- the scan of u32 counts
struct ScanU32 {
  static constexpr int WEIGHTS = 1;
  const uint32_t* v;
  uint64_t n;
  uint64_t* out;
  __device__ void weigh(uint64_t i, uint64_t* w) const { *w = i < n ? v[i] : 0; }
  __device__ void place(uint64_t i, uint64_t, uint64_t ex) const {
    if (i < n) out[i] = ex;
  }
};

// ---------------------------------------------------------------- rows
__global__ void __launch_bounds__(WG) k_vt_rows(VoteStore v, VoteCall c, const u64* __restrict__ item, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool brk = false;
  if (i < c.n && c.keyoff[i] != mvk::IX_NO_SRC) {
    const u64 it = item[i], code = code_of(it);
    const uint64_t p = it & SLOT_MASK;
    if (!item_has_slot(it) || p > v.t.mask) {
      vt_err(ctl);
    } else if (code == C_NEW) {
      const uint32_t nst = c.n_st[i];
      const u64 row = atomicAdd(ctl + mvk::VT_CTL_NROWS, 1ull);
      const u64 base = atomicAdd(ctl + mvk::VT_CTL_NCELLS, (u64)nst);
      if (row < v.cap_rows && base <= v.cap_cells && nst <= v.cap_cells - base) {
#pragma unroll
        for (int w = 0; w < 6; w++) v.row_key[6 * row + w] = c.key[6 * i + w];
        v.row_base[row] = base;
        v.row_n[row] = nst;
        v.row_agg[row] = 0;
        v.rowmap[p] = (uint32_t)row;
      } else {
        v.rowmap[p] = VT_NO_ROW;
        vt_err(ctl);
      }
    } else {
      brk = true;
      c.brk[i] = 1;
    }
  }
  wave_count_to(ctl + mvk::VT_CTL_NBRK, brk);
}

// ---------------------------------------------------------------- events
struct EmitF {
  const VoteStore& v;
  const VoteCall& c;
  u64* ctl;
  uint64_t i;
  bool votes;
  uint32_t own_row, own_n;  // VT_NO_ROW: the block registers nothing
  uint64_t reg_at, vote_at, reg_end, vote_end;
  uint64_t run0 = ~0ull, run1 = 0, unk = 0;
  uint32_t flags = 0;

  __device__ void put(uint64_t at, uint64_t lim, uint32_t row, uint32_t kind, uint64_t s, uint64_t e) {
    if (at >= lim || at >= c.cap_ev) {
      vt_err(ctl);
      return;
    }
    c.ev[3 * at] = row | ((u64)kind << 32);
    c.ev[3 * at + 1] = s | (e << 32);
    c.ev[3 * at + 2] = c.author[i] | ((u64)i << 32);
    c.evc[at] = 0;
    c.evx[at] = 0;
  }
  // the Share run in hand becomes a register event (runs are counted by ScanF in the same way)
  __device__ void flush() {
    if (run0 == ~0ull) return;
    uint64_t s = run0, e = run1;
    run0 = ~0ull;
    uint32_t kind = mvk::VT_KIND_REG;
    if (own_row == VT_NO_ROW) s = e = 0;
    if (e > own_n) {
      flags |= MV_VOTES_FLAG_REF_REUSED;
      e = own_n;
      s = s < e ? s : e;
    }
    if (s == e) kind = mvk::VT_KIND_NONE;
    put(reg_at++, reg_end, kind ? own_row : 0, kind, s, e);
  }
  __device__ void share(uint64_t k) {
    if (run0 == ~0ull) run0 = k;
    run1 = k + 1;
  }
  __device__ void target(const uint64_t* key, uint64_t s, uint64_t e) {
    bool fail;
    uint32_t probe, row = VT_NO_ROW, kind = mvk::VT_KIND_VOTE;
    const u64 p = find_slot(v.t, key, &probe, &fail);
    if (p != DG_NO_SLOT) row = v.rowmap[p];
    if (fail) vt_err(ctl);
    uint64_t cs = 0, ce = 0;
    if (row != VT_NO_ROW && row < v.cap_rows) {
      const uint64_t rn = v.row_n[row];
      ce = e < rn ? e : rn;
      cs = s < ce ? s : ce;
    }
    unk += (e - s) - (ce - cs);
    if (cs == ce) kind = mvk::VT_KIND_NONE, row = 0;
    put(vote_at++, vote_end, row, kind, cs, ce);
  }
  // (with MV_VOTES_REGISTER_ONLY the scan counted no vote events: none is written)
  __device__ void vote(uint64_t, const uint64_t* key, uint64_t lo) {
    flush();
    if (votes && vote_kind(lo) == 1) target(key, lo, lo + 1);
  }
  __device__ void reject(uint64_t) { flush(); }
  __device__ void range(uint64_t, const uint64_t* key, uint64_t s0, uint64_t s1) {
    flush();
    if (votes && range_kind(s0, s1) == 1) target(key, s0, s1);
  }
};

__device__ inline void emit_block(EmitF& f, const VoteCall& c, uint64_t i, u64* ctl) {
  BcReader r{c.buf + c.off[i], c.len[i], 0, true};
  // (the scan's walk parsed this block: byte 56 is its include count, its statements follow them)
  const uint64_t n_inc = ld64(r.p + br::INC_COUNT_OFF);
  if (!br::inc_count_readable(r.len) || !br::includes_inside(r.len, n_inc)) {
    vt_err(ctl);
    return;
  }
  r.pos = br::INC_OFF + br::REF_BYTES * n_inc;
  uint64_t count;
  if (!walk_statements(r, f, &count)) vt_err(ctl);
  f.flush();
  if (f.reg_at != f.reg_end || f.vote_at != f.vote_end) vt_err(ctl);  // the two walks disagree
  c.unk[i] = f.unk;
  c.bflags[i] |= f.flags;
}

__global__ void __launch_bounds__(WG) k_vt_emit(VoteStore v, VoteCall c, const u64* __restrict__ item, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= c.n || c.status[i] != MV_VOTES_OK || !block_span_ok(c, i)) return;
  uint32_t own_row = VT_NO_ROW, own_n = 0;
  if (c.keyoff[i] != mvk::IX_NO_SRC) {
    const uint64_t p = item[i] & SLOT_MASK;
    if (item_has_slot(item[i]) && p <= v.t.mask) own_row = v.rowmap[p];
    if (own_row != VT_NO_ROW && own_row < v.cap_rows) own_n = v.row_n[own_row];
    else own_row = VT_NO_ROW;
  }
  const uint64_t b = c.evbase[i], nreg = c.nreg[i], nev = c.nev[i];
  EmitF f{v, c, ctl, i, !(c.flags & MV_VOTES_REGISTER_ONLY), own_row, own_n, b, b + nreg, b + nreg, b + nev};
  emit_block(f, c, i, ctl);
}

// ---------------------------------------------------------------- a segment: group by row
__device__ inline uint32_t ev_row(const VoteCall& c, uint64_t e) { return (uint32_t)c.ev[3 * e]; }
__device__ inline uint32_t ev_kind(const VoteCall& c, uint64_t e) { return (uint32_t)(c.ev[3 * e] >> 32); }

__global__ void __launch_bounds__(WG) k_vt_count(VoteCall c, uint64_t e0, uint64_t e1, uint64_t nrows,
                                                 uint32_t* __restrict__ row_cnt, u64* __restrict__ ctl) {
  const uint64_t e = e0 + (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (e >= e1 || ev_kind(c, e) == mvk::VT_KIND_NONE) return;
  const uint32_t row = ev_row(c, e);
  if (row < nrows) atomicAdd(row_cnt + row, 1u);
  else vt_err(ctl);
}
__global__ void __launch_bounds__(WG) k_vt_scatter(VoteCall c, uint64_t e0, uint64_t e1, uint64_t nrows, VoteSeg g,
                                                   u64* __restrict__ ctl) {
  const uint64_t e = e0 + (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (e >= e1 || ev_kind(c, e) == mvk::VT_KIND_NONE) return;
  const uint32_t row = ev_row(c, e);
  if (row >= nrows) return;  // (counted by k_vt_count)
  const uint64_t pos = g.row_lb[row] + atomicAdd(g.row_cur + row, 1u);
  if (pos < e1 - e0) g.list[pos] = (uint32_t)(e - e0);
  else vt_err(ctl);
}
// a lane per list entry: its rank among its row's entries is its place (ids are distinct)
__global__ void __launch_bounds__(WG) k_vt_order(VoteCall c, uint64_t e0, uint64_t e1, uint64_t nrows, VoteSeg g,
                                                 u64* __restrict__ ctl) {
  const uint64_t p = (uint64_t)blockIdx.x * WG + threadIdx.x, L = e1 - e0;
  if (p >= L || p >= ctl[mvk::VT_CTL_NLIST]) return;
  const uint32_t me = g.list[p];
  if (me >= L) return vt_err(ctl);
  const uint32_t row = ev_row(c, e0 + me);
  if (row >= nrows) return vt_err(ctl);
  const uint64_t b = g.row_lb[row], cnt = g.row_cnt[row];
  if (b > L || cnt > L - b) return vt_err(ctl);
  uint64_t rank = 0;
  for (uint64_t j = 0; j < cnt; j++) rank += g.list[b + j] < me;
  g.sorted[b + rank] = me;
}

// ---------------------------------------------------------------- apply
__device__ inline uint32_t wave_sum32(uint32_t x) {
  for (int d = 32; d; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d);
  return x;
}

// A wave per row, its events one after another (committee.rs:364-425 per cell). Lane l of an event
// takes the offsets start + l, start + l + 64, ...: a cell is touched by one lane per event, and
// the wave's events are ordered by wave_sync.
__global__ void __launch_bounds__(WG) k_vt_apply(VoteStore v, VoteCall c, uint64_t nrows, uint64_t e0, uint64_t e1,
                                                 VoteSeg g, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t row = (uint64_t)blockIdx.x * (WG / 64) + threadIdx.x / 64, L = e1 - e0;
  if (row >= nrows) return;
  const uint64_t cnt = g.row_cnt[row], b = g.row_lb[row];
  if (cnt == 0) return;
  const uint64_t base = v.row_base[row], rn = v.row_n[row];
  if (b > L || cnt > L - b || base > v.cap_cells || rn > v.cap_cells - base) {
    if (lane == 0) vt_err(ctl);
    return;
  }
  const uint32_t nw = v.cw - 2;
  int32_t dagg = 0;
  for (uint64_t j = 0; j < cnt; j++) {
    const uint32_t rel = g.sorted[b + j];
    if (rel >= L) {
      if (lane == 0) vt_err(ctl);
      continue;
    }
    const uint64_t e = e0 + rel;
    const u64 w0 = c.ev[3 * e], w1 = c.ev[3 * e + 1], w2 = c.ev[3 * e + 2];
    const uint32_t kind = (uint32_t)(w0 >> 32), voter = (uint32_t)w2;
    const uint64_t start = (uint32_t)w1, end = w1 >> 32;
    if ((uint32_t)w0 != row || start > end || end > rn || voter >= c.n_auth || 2 + (voter >> 6) >= v.cw) {
      if (lane == 0) vt_err(ctl);
      continue;
    }
    const uint64_t stake = c.stakes[voter], bit = 1ull << (voter & 63), mark = (e + 1) << 1;
    const uint32_t vw = 2 + (voter >> 6);
    uint32_t ncert = 0, nx = 0;
    for (uint64_t o = start + lane; o < end; o += 64) {
      uint64_t* cell = v.cells + (base + o) * v.cw;
      const bool live = cell[0] == 1;
      if (kind == mvk::VT_KIND_REG) {
        if (live) {
          nx++;
        } else {  // (the voter words of an empty cell are zero)
          cell[0] = 1, cell[1] = stake, cell[vw] = bit;
          dagg++;
        }
      } else if (!live) {
        nx++;
      } else {
        const u64 vs = cell[vw];
        u64 sum = cell[1];
        if (!(vs & bit)) {
          sum += stake;
          cell[vw] = vs | bit, cell[1] = sum;
        }
        if (sum >= c.quorum) {
          cell[0] = mark, cell[1] = 0;
          for (uint32_t k = 0; k < nw; k++) cell[2 + k] = 0;
          ncert++;
          dagg--;
        }
      }
    }
    ncert = wave_sum32(ncert), nx = wave_sum32(nx);
    if (lane == 0) c.evc[e] = ncert, c.evx[e] = nx;
    wave_sync();
  }
  dagg = (int32_t)wave_sum32((uint32_t)dagg);
  if (lane == 0) v.row_agg[row] += (uint32_t)dagg;
}

// A wave per event that certified: its cells carry its mark; their rows go out in ascending offset
// behind the event's base, and the marks are cleared.
__global__ void __launch_bounds__(WG) k_vt_certs(VoteStore v, VoteCall c, uint64_t nrows, uint64_t e0, uint64_t e1,
                                                 VoteSeg g, uint64_t* __restrict__ out, uint64_t cap, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t e = e0 + (uint64_t)blockIdx.x * (WG / 64) + threadIdx.x / 64;
  if (e >= e1 || c.evc[e] == 0) return;
  const u64 w0 = c.ev[3 * e], w1 = c.ev[3 * e + 1], w2 = c.ev[3 * e + 2];
  const uint64_t row = (uint32_t)w0, start = (uint32_t)w1, end = w1 >> 32;
  if (row >= nrows) return;  // (k_vt_apply gave such an event no count)
  const uint64_t base = v.row_base[row], rn = v.row_n[row];
  if (start > end || end > rn || base > v.cap_cells || rn > v.cap_cells - base) return;
  const u64 mark = (e + 1) << 1;
  uint64_t at = g.certbase[e - e0];
  for (uint64_t o0 = start; o0 < end; o0 += 64) {
    const uint64_t o = o0 + lane;
    uint64_t* cell = v.cells + (base + o) * v.cw;
    const bool mine = o < end && __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mark;
    const u64 m = __ballot(mine);
    if (mine) {
      const uint64_t pos = at + __popcll(m & ((1ull << lane) - 1));
      if (pos < cap) {
#pragma unroll
        for (int w = 0; w < 6; w++) out[8 * pos + w] = v.row_key[6 * row + w];
        out[8 * pos + 6] = o;
        out[8 * pos + 7] = w2 >> 32;
      }
      __hip_atomic_store(cell, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    at += __popcll(m);
  }
}

__global__ void __launch_bounds__(WG) k_vt_blockout(VoteCall c, uint64_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= c.n) return;
  uint64_t cert = 0, unk = c.unk[i], dup = 0;
  const uint64_t b = c.evbase[i], nreg = c.nreg[i], nev = c.nev[i];
  if (b <= c.cap_ev && nev <= c.cap_ev - b) {
    for (uint64_t k = 0; k < nev; k++) {
      cert += c.evc[b + k];
      if (k < nreg) dup += c.evx[b + k];
      else unk += c.evx[b + k];
    }
  }
  counts[4 * i] = cert, counts[4 * i + 1] = unk, counts[4 * i + 2] = dup, counts[4 * i + 3] = c.bflags[i];
}

__global__ void __launch_bounds__(WG) k_vt_stats(VoteStore v, uint64_t nrows, u64* __restrict__ ctl) {
  const uint64_t row = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const uint32_t agg = row < nrows ? v.row_agg[row] : 0;
  wave_count_to(ctl + mvk::VT_CTL_PENDING, agg != 0);
  const uint64_t a = wave_sum64(agg), l = wave_sum64(agg ? v.row_n[row] : 0);
  if ((threadIdx.x & 63) == 0 && a) {
    atomicAdd(ctl + mvk::VT_CTL_AGG, (u64)a);
    atomicAdd(ctl + mvk::VT_CTL_LIVECELLS, (u64)l);
  }
}

// A wave per row of v with an aggregating cell: a row, a run of cells and a slot in q (keys are
// distinct: the first empty slot is claimed and nothing compares, as k_ix_rebuild).
__global__ void __launch_bounds__(WG) k_vt_move(VoteStore v, uint64_t nrows, VoteStore q, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t row = (uint64_t)blockIdx.x * (WG / 64) + threadIdx.x / 64;
  if (row >= nrows || v.row_agg[row] == 0) return;
  const uint64_t base = v.row_base[row], rn = v.row_n[row];
  if (base > v.cap_cells || rn > v.cap_cells - base || v.cw != q.cw) {
    if (lane == 0) vt_err(ctl);
    return;
  }
  uint64_t nr = 0, nb = 0;
  if (lane == 0) {
    nr = atomicAdd(ctl + mvk::VT_CTL_NROWS, 1ull);
    nb = atomicAdd(ctl + mvk::VT_CTL_NCELLS, (u64)rn);
  }
  nr = shfl64(nr, 0), nb = shfl64(nb, 0);
  if (nr >= q.cap_rows || nb > q.cap_cells || rn > q.cap_cells - nb) {
    if (lane == 0) vt_err(ctl);
    return;
  }
  if (lane == 0) {
    uint64_t k[6];
#pragma unroll
    for (int w = 0; w < 6; w++) k[w] = v.row_key[6 * row + w];
    uint32_t probe;
    const u64 p = claim_fresh(q.t, k, 1, &probe);
    if (p != DG_NO_SLOT) q.rowmap[p] = (uint32_t)nr;
    else vt_err(ctl);
#pragma unroll
    for (int w = 0; w < 6; w++) q.row_key[6 * nr + w] = k[w];
    q.row_base[nr] = nb;
    q.row_n[nr] = (uint32_t)rn;
    q.row_agg[nr] = v.row_agg[row];
  }
  const uint64_t words = rn * v.cw;
  for (uint64_t w = lane; w < words; w += 64) q.cells[nb * q.cw + w] = v.cells[base * v.cw + w];
}

}  // namespace
}  // namespace mv::ix

namespace mvk {
using namespace mv::ix;

hipError_t launch_votes_scan_u32(const uint32_t* v, uint64_t n, uint64_t* out, uint64_t* total, uint64_t* running,
                                 void* wg, hipStream_t s) {
  if (n == 0) {
    if (hipMemsetAsync(total, 0, 8, s) != hipSuccess) return hipGetLastError();
    return hipSuccess;
  }
  compact_pass(ScanU32{v, n, out}, n, wg_scan_of(wg, n), total, nullptr, running, s);
  return hipGetLastError();
}

hipError_t launch_votes_scan(const VoteCall& c, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_vt_scan, dim3(grid_of(c.n)), dim3(WG), 0, s, c, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_votes_rows(const VoteStore& v, const VoteCall& c, const uint64_t* item, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_vt_rows, dim3(grid_of(c.n)), dim3(WG), 0, s, v, c, (const u64*)item, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_votes_emit(const VoteStore& v, const VoteCall& c, const uint64_t* item, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_vt_emit, dim3(grid_of(c.n)), dim3(WG), 0, s, v, c, (const u64*)item, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_votes_segment(const VoteStore& v, const VoteCall& c, uint64_t nrows, uint64_t e0, uint64_t e1,
                                const VoteSeg& g, uint64_t* certified, uint64_t cap_cert, uint64_t* ctl, hipStream_t s) {
  if (e1 <= e0 || nrows == 0) return hipSuccess;
  const uint64_t L = e1 - e0;
  u64* cw = reinterpret_cast<u64*>(ctl);
  const dim3 b(WG), ge(grid_of(L)), gw(grid_of(L * 64)), gr(grid_of(nrows * 64));
  if (hipMemsetAsync(g.row_cnt, 0, 4 * nrows, s) != hipSuccess || hipMemsetAsync(g.row_cur, 0, 4 * nrows, s) != hipSuccess)
    return hipGetLastError();
  hipLaunchKernelGGL(k_vt_count, ge, b, 0, s, c, e0, e1, nrows, g.row_cnt, cw);
  (void)launch_votes_scan_u32(g.row_cnt, nrows, g.row_lb, ctl + VT_CTL_NLIST, nullptr, g.wg, s);
  hipLaunchKernelGGL(k_vt_scatter, ge, b, 0, s, c, e0, e1, nrows, g, cw);
  hipLaunchKernelGGL(k_vt_order, ge, b, 0, s, c, e0, e1, nrows, g, cw);
  hipLaunchKernelGGL(k_vt_apply, gr, b, 0, s, v, c, nrows, e0, e1, g, cw);
  (void)launch_votes_scan_u32(c.evc + e0, L, g.certbase, ctl + VT_CTL_SEGCERT, ctl + VT_CTL_NCERT, g.wg, s);
  hipLaunchKernelGGL(k_vt_certs, gw, b, 0, s, v, c, nrows, e0, e1, g, certified, cap_cert, cw);
  return hipGetLastError();
}

hipError_t launch_votes_blockout(const VoteCall& c, uint64_t* blk_counts, hipStream_t s) {
  hipLaunchKernelGGL(k_vt_blockout, dim3(grid_of(c.n)), dim3(WG), 0, s, c, blk_counts);
  return hipGetLastError();
}

hipError_t launch_votes_stats(const VoteStore& v, uint64_t nrows, uint64_t* ctl, hipStream_t s) {
  if (nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vt_stats, dim3(grid_of(nrows)), dim3(WG), 0, s, v, nrows, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_votes_move(const VoteStore& v, uint64_t nrows, const VoteStore& q, uint64_t* ctl, hipStream_t s) {
  if (nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vt_move, dim3(grid_of(nrows * 64)), dim3(WG), 0, s, v, nrows, q, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
