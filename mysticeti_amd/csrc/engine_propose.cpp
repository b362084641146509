// libmysti_verify.so: the proposer's state (mv_propose_reserve, mv_propose_add, mv_propose_take,
// mv_propose_own, mv_propose_stats): the host side of propose.hip.
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

using namespace mvi;

namespace {
constexpr uint64_t kMaxProposeRows = 0xfffffffeull;  // a row's number is a u32 (all ones: none)
constexpr size_t kEntryBytes = 28;                   // slot | round | tag (u64), kind (u32)

// the queue's copy k as the kernels see it
mvk::PropQueue queue_view(const DevBuf& b, uint64_t cap) {
  char* p = b.as<char>();
  return mvk::PropQueue{(uint32_t*)(p + 24 * cap), (uint64_t*)p, (uint64_t*)(p + 8 * cap), (uint64_t*)(p + 16 * cap)};
}
mvk::PropQueue queue_view(const Propose& pp, int k) { return queue_view(pp.q[k], pp.cap); }

// Room in the queue for `more` entries on top of those there: two fresh copies, at least twice as
// large, of which the first takes the entries over. Synchronises s when it grows.
mv_status queue_room(mv_ctx* ctx, Device& dev, uint64_t more, hipStream_t s) {
  Propose& pp = dev.index.prop;
  const uint64_t need = pp.qn + more;
  if (need <= pp.cap) return MV_OK;
  if (need > kMaxProposeRows) return set_err(ctx, MV_E_INVALID_ARG, "too many entries in the proposer's queue");
  const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * pp.cap), 64);
  DevBuf a, b;
  if (a.ensure(kEntryBytes * (size_t)cap) != hipSuccess || b.ensure(kEntryBytes * (size_t)cap) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "no device memory for the proposer's queue");
  }
  if (pp.qn) {
    const mvk::PropQueue from = queue_view(pp, pp.cur), to = queue_view(a, cap);
    HIPCHK(ctx, hipMemcpyAsync(to.slot, from.slot, 8 * (size_t)pp.qn, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.round, from.round, 8 * (size_t)pp.qn, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.tag, from.tag, 8 * (size_t)pp.qn, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.kind, from.kind, 4 * (size_t)pp.qn, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));  // the old copies are read until here; a and b free them below
  std::swap(pp.q[pp.cur], a);
  std::swap(pp.q[pp.cur ^ 1], b);
  pp.cap = cap;
  return MV_OK;
}

// the state's control words on the host, with the index's (synchronises s)
mv_status read_pctl(mv_ctx* ctx, Device& dev, hipStream_t s, uint64_t* w) {
  Propose& pp = dev.index.prop;
  HIPCHK(ctx, hipMemcpyAsync(w, pp.ctl.p, 8 * mvk::PP_CTL_WORDS, hipMemcpyDeviceToHost, s));
  const mv_status st = read_ctl(ctx, dev, s, nullptr);
  if (st == MV_OK) pp.round = w[mvk::PP_CTL_ROUND];
  return st;
}
mv_status zero_call_words(mv_ctx* ctx, Propose& pp, hipStream_t s) {
  HIPCHK(ctx, hipMemsetAsync(pp.ctl.as<uint64_t>() + mvk::PP_CTL_NMISS, 0, 8 * (mvk::PP_CTL_WORDS - mvk::PP_CTL_NMISS), s));
  return MV_OK;
}

// a call's per-row scratch, carved from pp.rows
struct RowScratch {
  uint64_t *slot, *round, *stot;
  uint32_t *auth, *sauth, *perm[2], *seglen, *pos0, *pos1;
  uint8_t* first;
};
mv_status row_scratch(mv_ctx* ctx, Propose& pp, uint64_t n, RowScratch& r) {
  const size_t a64 = ix_al(8 * n), a32 = ix_al(4 * n), a8 = ix_al(n);
  HIPCHK(ctx, pp.rows.ensure(3 * a64 + 7 * a32 + a8));
  char* b = pp.rows.as<char>();
  r.slot = (uint64_t*)b, r.round = (uint64_t*)(b + a64), r.stot = (uint64_t*)(b + 2 * a64);
  b += 3 * a64;
  r.auth = (uint32_t*)b, r.sauth = (uint32_t*)(b + a32), r.perm[0] = (uint32_t*)(b + 2 * a32), r.perm[1] = (uint32_t*)(b + 3 * a32);
  r.seglen = (uint32_t*)(b + 4 * a32), r.pos0 = (uint32_t*)(b + 5 * a32), r.pos1 = (uint32_t*)(b + 6 * a32);
  r.first = (uint8_t*)(b + 7 * a32);
  return MV_OK;
}

// ThresholdClockAggregator::add_block over n rows (rounds and authorities in device memory), in order
mv_status clock_run(mv_ctx* ctx, Device& dev, const uint64_t* d_round, const uint32_t* d_auth, uint64_t n, const RowScratch& r,
                    hipStream_t s) {
  Propose& pp = dev.index.prop;
  const mvh::Committee& com = ctx->committee;
  const mvk::PropClock c{d_round, d_auth, n, r.first, r.seglen, r.pos0, r.pos1, r.stot, dev.tab.stakes.as<uint64_t>(),
                         com.size(), com.quorum_threshold};
  HIPCHK(ctx, mvk::launch_propose_clock(c, pp.ctl.as<uint64_t>(), dev.index.ctl.as<uint64_t>(), s));
  return MV_OK;
}

// One add call on stream s (include/mysti_verify.h, mv_propose_add); the rows and tags are device
// memory. Synchronises s: the rows without a slot decide whether anything changes, their rounds size the
// sort, and the clock is read back. res: the four words of `out`.
mv_status add_run(mv_ctx* ctx, Device& dev, const uint64_t* d_rows, uint64_t n, uint64_t stride, const uint64_t* d_tags,
                  uint32_t flags, uint64_t token, hipStream_t s, uint64_t* res) {
  Index& ix = dev.index;
  Propose& pp = ix.prop;
  const bool payload = flags & MV_PROPOSE_PAYLOAD;
  mv_status st = index_ctl(ctx, dev, s);
  if (st == MV_OK) st = zero_call_words(ctx, pp, s);
  if (st != MV_OK) return st;
  uint64_t* pctl = pp.ctl.as<uint64_t>();
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  uint64_t w[mvk::PP_CTL_WORDS];
  RowScratch r{};
  if (n) {
    st = row_scratch(ctx, pp, n, r);
    if (st != MV_OK) return st;
    HIPCHK(ctx, mvk::launch_propose_resolve(table_of(ctx, ix), d_rows, n, stride, ctx->committee.size(), r.slot, r.round, r.auth,
                                            r.perm[0], pctl, ctl, s));
    st = read_pctl(ctx, dev, s, w);
    if (st != MV_OK) return st;
    if (w[mvk::PP_CTL_NMISS])
      return set_err(ctx, MV_E_INVALID_ARG,
                     "propose_add: " + std::to_string(w[mvk::PP_CTL_NMISS]) +
                         " rows are not in the index or name an authority outside the committee");
  }
  st = queue_room(ctx, dev, n + (payload ? 1 : 0), s);
  if (st != MV_OK) return st;
  int cur = 0;
  if (n && !(flags & MV_PROPOSE_IN_ORDER)) {
    // the stable sort by round (core.rs:181-183): an LSD pass for every bit that is 1 in one row's
    // round and 0 in another's (a bit that is the same in all rows cannot order two of them)
    const uint64_t differ = w[mvk::PP_CTL_OR] & w[mvk::PP_CTL_NOR];
    HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(n)));
    for (int bit = 0; bit < 64; bit++) {
      if (!((differ >> bit) & 1)) continue;
      HIPCHK(ctx, mvk::launch_propose_sort_bit(r.round, bit, r.perm[cur], r.perm[cur ^ 1], n, ix.wg.as<uint64_t>(), pctl, s));
      cur ^= 1;
    }
  }
  const mvk::PropQueue q = queue_view(pp, pp.cur);
  HIPCHK(ctx, mvk::launch_propose_append(r.slot, r.round, r.auth, d_tags, r.perm[cur], n, q, pp.qn, pp.cap, r.sauth, payload,
                                         token, ctl, s));
  if (n) {
    st = clock_run(ctx, dev, q.round + pp.qn, r.sauth, n, r, s);
    if (st != MV_OK) return st;
  }
  st = read_pctl(ctx, dev, s, w);
  if (st != MV_OK) return st;
  pp.qn += n + (payload ? 1 : 0);
  res[0] = w[mvk::PP_CTL_ROUND], res[1] = w[mvk::PP_CTL_STAKE], res[2] = w[mvk::PP_CTL_VOTERS], res[3] = pp.qn;
  return MV_OK;
}

mv_status check_add(mv_ctx* ctx, const void* rows, uint64_t n, uint64_t stride, uint32_t flags, const void* out) {
  if (!ctx || !out || (n && !rows) || stride < 6 || n > kMaxProposeRows || (flags & ~(uint32_t)(MV_PROPOSE_IN_ORDER | MV_PROPOSE_PAYLOAD)))
    return set_err(ctx, MV_E_INVALID_ARG, "bad propose_add args");
  return MV_OK;
}
mv_status need_state(mv_ctx* ctx, Device& dev) {
  if (!dev.index.prop.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_propose_reserve first");
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  return MV_OK;
}
}  // namespace

mv_status mvi::propose_follow_table(mv_ctx* ctx, Device& dev, uint64_t old_slots, const mvk::IndexTable& nt, hipStream_t s) {
  Index& ix = dev.index;
  Propose& pp = ix.prop;
  const uint64_t* old = ix.tab.as<uint64_t>();
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  if (pp.qn) HIPCHK(ctx, mvk::launch_index_reresolve(old, old_slots, nt, queue_view(pp, pp.cur).slot, pp.qn, ctl, s));
  if (pp.has_own)
    HIPCHK(ctx, mvk::launch_index_reresolve(old, old_slots, nt, pp.own[pp.own_cur].as<uint64_t>(), 1 + pp.own_k, ctl, s));
  if (pp.outstanding && pp.n_choice)
    HIPCHK(ctx, mvk::launch_index_reresolve(old, old_slots, nt, pp.choice.as<uint64_t>(), pp.n_choice, ctl, s));
  pp.stamp_slots = 0;  // the stamps are per slot of the table: remade and zeroed by the next take
  return MV_OK;
}

mv_status mvi::propose_clear(mv_ctx* ctx, Device& dev, hipStream_t s) {
  Propose& pp = dev.index.prop;
  pp.qn = pp.own_k = pp.n_choice = pp.own_round = pp.take_round = pp.round = 0;
  pp.has_own = pp.outstanding = false;
  pp.takes = pp.dropped = 0;
  pp.stamp_slots = 0;
  HIPCHK(ctx, hipMemsetAsync(pp.ctl.p, 0, 8 * mvk::PP_CTL_WORDS, s));
  return MV_OK;
}

extern "C" {

mv_status mv_propose_reserve(mv_ctx* ctx, uint32_t authority, uint64_t entries) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  if (authority >= ctx->committee.size() || ctx->committee.size() > mvk::DG_MAX_AUTH)
    return set_err(ctx, MV_E_INVALID_ARG, "propose_reserve: the authority is not one of the committee's (of at most 512 seats)");
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Propose& pp = dev->index.prop;
  hipStream_t s = dev->stream;
  if (pp.on && pp.authority != authority && (pp.has_own || pp.qn))
    return set_err(ctx, MV_E_INVALID_ARG, "propose_reserve: reserved for another authority (mv_index_clear empties the state)");
  pp.authority = authority;
  st = index_ctl(ctx, *dev, s);
  if (st != MV_OK) return st;
  if (!pp.on) {
    HIPCHK(ctx, pp.ctl.ensure(8 * mvk::PP_CTL_WORDS));
    HIPCHK(ctx, hipMemsetAsync(pp.ctl.p, 0, 8 * mvk::PP_CTL_WORDS, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    pp.authority = authority;
    pp.on = true;
  }
  return queue_room(ctx, *dev, entries > pp.qn ? entries - pp.qn : 0, s);
}

mv_status mv_propose_add(mv_ctx* ctx, const uint64_t* rows, uint64_t n, uint64_t stride_words, const uint64_t* tags,
                         uint32_t flags, uint64_t payload_token, uint64_t* out) {
  mv_status st = check_add(ctx, rows, n, stride_words, flags, out);
  if (st != MV_OK) return st;
  memset(out, 0, 4 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  st = index_dev(ctx, dev);
  if (st == MV_OK) st = need_state(ctx, *dev);
  if (st != MV_OK) return st;
  Propose& pp = dev->index.prop;
  hipStream_t s = dev->stream;
  const uint64_t* d_rows = nullptr;
  const uint64_t* d_tags = nullptr;
  if (n) {
    const size_t rb = 8 * (size_t)n * stride_words;
    HIPCHK(ctx, pp.in.ensure(ix_al(rb) + 8 * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(pp.in.p, rows, rb, hipMemcpyHostToDevice, s));
    d_rows = pp.in.as<uint64_t>();
    if (tags) {
      HIPCHK(ctx, hipMemcpyAsync(pp.in.as<char>() + ix_al(rb), tags, 8 * (size_t)n, hipMemcpyHostToDevice, s));
      d_tags = (const uint64_t*)(pp.in.as<char>() + ix_al(rb));
    }
  }
  st = add_run(ctx, *dev, d_rows, n, stride_words, d_tags, flags, payload_token, s, out);
  if (st != MV_OK) (void)hipStreamSynchronize(s);
  return st;
}

mv_status mv_dev_propose_add(mv_ctx* ctx, int device, const uint64_t* d_rows, uint64_t n, uint64_t stride_words,
                             const uint64_t* d_tags, uint32_t flags, uint64_t payload_token, uint64_t* d_out, void* stream) {
  mv_status st = check_add(ctx, d_rows, n, stride_words, flags, d_out);
  if (st != MV_OK) return st;
  if ((((uintptr_t)d_rows) & 7) || (((uintptr_t)d_tags) & 7) || (((uintptr_t)d_out) & 7))
    return set_err(ctx, MV_E_INVALID_ARG, "d_rows, d_tags and d_out must be 8-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  st = need_state(ctx, *dev);
  if (st != MV_OK) return st;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  uint64_t res[4] = {0, 0, 0, 0};
  st = add_run(ctx, *dev, d_rows, n, stride_words, d_tags, flags, payload_token, s, res);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(d_out, res, sizeof(res), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return MV_OK;
}

mv_status mv_propose_take(mv_ctx* ctx, uint64_t* includes, uint64_t cap, uint64_t* n_includes, uint64_t* payloads,
                          uint64_t cap_p, uint64_t* n_payloads, uint64_t* out) {
  if (!ctx || !n_includes || !n_payloads || !out || (cap && !includes) || (cap_p && !payloads))
    return set_err(ctx, MV_E_INVALID_ARG, "bad propose_take args");
  *n_includes = *n_payloads = 0;
  memset(out, 0, 6 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st == MV_OK) st = need_state(ctx, *dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  Propose& pp = ix.prop;
  Dag& dg = ix.dag;
  hipStream_t s = dev->stream;
  if (!pp.has_own) return set_err(ctx, MV_E_INVALID_ARG, "propose_take: no own last block (mv_propose_own first)");
  if (pp.outstanding) return set_err(ctx, MV_E_INVALID_ARG, "propose_take: a take is outstanding (mv_propose_own confirms it)");
  const uint64_t R = pp.round;
  out[1] = R, out[4] = ~0ull, out[5] = pp.qn;
  if (R <= pp.own_round) return MV_OK;  // (core.rs:233-235)
  if (!ix.slots) return set_err(ctx, MV_E_HIP, "propose_take: an own last block without an index");
  uint64_t* pctl = pp.ctl.as<uint64_t>();
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  // the stamps: as long as the table; a fresh call number stands for an empty set
  if (pp.stamp_slots != ix.slots || pp.counter == 0xffffffffu) {
    HIPCHK(ctx, pp.stamp.ensure(4 * (size_t)ix.slots));
    HIPCHK(ctx, hipMemsetAsync(pp.stamp.p, 0, 4 * (size_t)ix.slots, s));
    pp.stamp_slots = ix.slots;
    pp.counter = 0;
  }
  const uint32_t counter = ++pp.counter;
  st = zero_call_words(ctx, pp, s);
  if (st != MV_OK) return st;
  HIPCHK(ctx, hipMemsetAsync(pctl + mvk::PP_CTL_CUT, 0xff, 8, s));
  const mvk::PropQueue q = queue_view(pp, pp.cur);
  uint64_t w[mvk::PP_CTL_WORDS];
  HIPCHK(ctx, mvk::launch_propose_cut(q, pp.qn, R, pctl, s));
  st = read_pctl(ctx, *dev, s, w);
  if (st != MV_OK) return st;
  const uint64_t cut = std::min<uint64_t>(w[mvk::PP_CTL_CUT], pp.qn);
  const bool dag_on = dg.on && dg.map_slots == ix.slots && dg.map.p;
  const mvk::DagStore d = dag_on ? dag_view(dg) : mvk::DagStore{};
  HIPCHK(ctx, mvk::launch_propose_stamp(q, cut, d, dg.nb, dag_on, pp.own[pp.own_cur].as<uint64_t>() + 1, pp.own_k, pp.stamp.as<uint32_t>(),
                                        pp.stamp_slots, counter, pctl, ctl, s));
  const uint64_t capd = std::min(cap, cut), cappd = std::min(cap_p, cut);
  HIPCHK(ctx, pp.res.ensure(ix_al(48 * (size_t)capd + 8) + 8 * (size_t)cappd + 8));
  HIPCHK(ctx, pp.choice.ensure(8 * (size_t)cut + 8));
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(cut ? cut : 1)));
  uint64_t* d_inc = pp.res.as<uint64_t>();
  uint64_t* d_pay = (uint64_t*)(pp.res.as<char>() + ix_al(48 * (size_t)capd + 8));
  HIPCHK(ctx, mvk::launch_propose_keep(table_of(ctx, ix), q, pp.qn, cut, pp.stamp.as<uint32_t>(), pp.stamp_slots, counter, d_inc,
                                       capd, pp.choice.as<uint64_t>(), cut, d_pay, cappd, ix.wg.as<uint64_t>(), pctl, ctl, s));
  st = read_pctl(ctx, *dev, s, w);
  if (st != MV_OK) return st;
  const uint64_t ninc = std::min<uint64_t>(w[mvk::PP_CTL_NINC], cut), npay = std::min<uint64_t>(w[mvk::PP_CTL_NPAY], cut);
  const uint64_t nent = std::min<uint64_t>(w[mvk::PP_CTL_NENT], cut);
  *n_includes = ninc, *n_payloads = npay;
  if (std::min(ninc, capd)) HIPCHK(ctx, hipMemcpyAsync(includes, d_inc, 48 * (size_t)std::min(ninc, capd), hipMemcpyDeviceToHost, s));
  if (std::min(npay, cappd)) HIPCHK(ctx, hipMemcpyAsync(payloads, d_pay, 8 * (size_t)std::min(npay, cappd), hipMemcpyDeviceToHost, s));
  out[2] = cut, out[3] = w[mvk::PP_CTL_FLAGS], out[4] = w[mvk::PP_CTL_NEXT];
  if (ninc > cap || npay > cap_p) {  // the totals alone: queue and state stay as they were
    out[3] |= MV_PROPOSE_SHORT;
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MV_OK;
  }
  HIPCHK(ctx, mvk::launch_propose_shift(q, queue_view(pp, pp.cur ^ 1), cut, pp.qn, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  pp.cur ^= 1;
  pp.qn -= cut;
  pp.outstanding = true;
  pp.take_round = R;
  pp.n_choice = ninc;
  pp.takes++;
  pp.dropped = nent - std::min(ninc, nent);
  out[0] = 1, out[5] = pp.qn;
  return MV_OK;
}

mv_status mv_propose_own(mv_ctx* ctx, const uint64_t* ref, const uint64_t* includes, uint64_t k, uint64_t* out) {
  if (!ctx || !ref || !out || (!includes && k) || k > kMaxProposeRows) return set_err(ctx, MV_E_INVALID_ARG, "bad propose_own args");
  memset(out, 0, 4 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st == MV_OK) st = need_state(ctx, *dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  Propose& pp = ix.prop;
  Dag& dg = ix.dag;
  hipStream_t s = dev->stream;
  const bool implicit = includes == nullptr;
  if (ref[0] != pp.authority) return set_err(ctx, MV_E_INVALID_ARG, "propose_own: the block is not the reserved authority's");
  if (implicit && (!pp.outstanding || !pp.has_own || ref[1] != pp.take_round))
    return set_err(ctx, MV_E_INVALID_ARG, "propose_own: no take outstanding at the block's round");
  const uint64_t kk = implicit ? 1 + pp.n_choice : k;
  // room first, so that a refusal leaves everything as it was: the table (may rebuild: the slots below
  // are read behind it), the DAG store for the record, the own array's other copy
  st = index_room_for_more(ctx, *dev, 1, /*can_grow=*/true, s);
  if (st == MV_OK && dg.on) {
    if (dg.map_slots != ix.slots) return set_err(ctx, MV_E_HIP, "the DAG store's map does not match the index");
    st = dag_room(ctx, *dev, 1, kk, s);
  }
  if (st == MV_OK) st = zero_call_words(ctx, pp, s);
  if (st != MV_OK) return st;
  DevBuf& own = pp.own[pp.own_cur ^ 1];
  HIPCHK(ctx, own.ensure(8 * (size_t)(kk + 2)));
  uint64_t* pctl = pp.ctl.as<uint64_t>();
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  uint64_t w[mvk::PP_CTL_WORDS];
  RowScratch r{};
  st = row_scratch(ctx, pp, std::max<uint64_t>(k, 1), r);
  if (st != MV_OK) return st;
  if (k) {
    HIPCHK(ctx, pp.in.ensure(48 * (size_t)k));
    HIPCHK(ctx, hipMemcpyAsync(pp.in.p, includes, 48 * (size_t)k, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, mvk::launch_propose_resolve(table_of(ctx, ix), pp.in.as<uint64_t>(), k, 6, ctx->committee.size(), r.slot, r.round,
                                            r.auth, r.perm[0], pctl, ctl, s));
    st = read_pctl(ctx, *dev, s, w);
    if (st != MV_OK) return st;
    if (w[mvk::PP_CTL_NMISS]) return set_err(ctx, MV_E_INVALID_ARG, "propose_own: an include is not in the index");
  }
  // 1. the reference: MV_REF_STORED
  HIPCHK(ctx, ix.keys.ensure(48));
  HIPCHK(ctx, hipMemcpyAsync(ix.keys.p, ref, 48, hipMemcpyHostToDevice, s));
  st = insert_rounds(ctx, *dev, mvk::IndexKeys{ix.keys.as<uint8_t>(), nullptr, 48, 0}, 1, MV_REF_STORED, s);
  if (st != MV_OK) return st;
  // 3. the own last block: its slot and its includes as slots
  HIPCHK(ctx, mvk::launch_propose_own(ix.item.as<uint64_t>(), implicit ? pp.own[pp.own_cur].as<uint64_t>() : nullptr, implicit,
                                      implicit ? pp.choice.as<uint64_t>() : r.slot, implicit ? pp.n_choice : k, own.as<uint64_t>(),
                                      ix.slots, ctl, s));
  // 2. add_block(ref) on the clock
  const uint32_t a32 = (uint32_t)ref[0];
  HIPCHK(ctx, hipMemcpyAsync(r.round, ref + 1, 8, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(r.sauth, &a32, 4, hipMemcpyHostToDevice, s));
  st = clock_run(ctx, *dev, r.round, r.sauth, 1, r, s);
  if (st != MV_OK) return st;
  // 5. its record, so that the committer and the linearizer see the block
  bool record = false;
  if (dg.on) {
    HIPCHK(ctx, mvk::launch_propose_record(table_of(ctx, ix), dag_view(dg), dg.nb, dg.ni, own.as<uint64_t>(), kk, pctl, ctl, s));
    record = true;
  }
  st = read_pctl(ctx, *dev, s, w);
  if (st != MV_OK) return st;
  if (record && w[mvk::PP_CTL_APPENDED]) dg.nb += 1, dg.ni += kk;
  pp.own_cur ^= 1;
  pp.has_own = true;
  pp.own_round = ref[1];
  pp.own_k = kk;
  pp.outstanding = false;  // 4.
  pp.n_choice = 0;
  out[0] = w[mvk::PP_CTL_ROUND], out[1] = w[mvk::PP_CTL_STAKE], out[2] = w[mvk::PP_CTL_VOTERS], out[3] = pp.qn;
  return MV_OK;
}

mv_status mv_propose_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad propose_stats args");
  memset(out, 0, 8 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Propose& pp = dev->index.prop;
  if (!pp.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_propose_reserve first");
  uint64_t w[mvk::PP_CTL_WORDS];
  st = read_pctl(ctx, *dev, dev->stream, w);
  if (st != MV_OK) return st;
  out[0] = w[mvk::PP_CTL_ROUND], out[1] = w[mvk::PP_CTL_STAKE], out[2] = w[mvk::PP_CTL_VOTERS], out[3] = pp.qn;
  out[4] = pp.has_own ? pp.own_round : 0, out[5] = pp.outstanding, out[6] = pp.takes, out[7] = pp.dropped;
  return MV_OK;
}

}  // extern "C"
