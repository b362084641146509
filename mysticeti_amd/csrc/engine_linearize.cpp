// libmysti_verify.so: the linearizer over the DAG store (mv_linearize, mv_linearize_mark,
// mv_linearize_stats): the host side of linearize.hip.
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

using namespace mvi;

namespace {
constexpr uint64_t kMaxLinearBuckets = 1ull << 24;

// One linearize call on stream s (include/mysti_verify.h, mv_linearize). The leaders are on the host
// (their rounds choose the levels) and on the device. Synchronises s for the store's lowest round
// (it bounds the buckets), for the edge counts per bucket (they size the edge list and every level's
// launches), behind each run of levels (4, 8, ... 64 of them: the lowest round still reachable ends the
// sweep), and for the call's totals (they move the context's counters). d_blocks == nullptr: the rows go to the
// context's own buffer, no longer than the call can fill, which *own_blocks then names.
mv_status linearize_run(mv_ctx* ctx, Device& dev, const uint64_t* leaders, const uint64_t* d_leaders, uint32_t n32,
                        uint64_t* d_blocks, uint64_t cap, uint64_t* d_sub, hipStream_t s, uint64_t* n_rows,
                        uint64_t** own_blocks = nullptr) {
  Index& ix = dev.index;
  Dag& dg = ix.dag;
  const size_t n = n32;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  if (!ix.slots || !dg.lmark.p) {  // no table yet: no leader has an entry
    std::vector<uint64_t> sub(4 * n, 0);
    for (size_t k = 0; k < n; k++) sub[4 * k] = k ? MV_LINEAR_STOPPED : MV_LINEAR_INCOMPLETE;
    HIPCHK(ctx, hipMemcpyAsync(d_sub, sub.data(), 32 * n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MV_OK;
  }
  if (dg.map_slots != ix.slots) return set_err(ctx, MV_E_HIP, "the DAG store's map does not match the index");
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  const uint64_t nb = dg.nb;
  uint64_t hi = 0;
  for (size_t k = 0; k < n; k++) hi = std::max(hi, leaders[6 * k + 1]);
  const uint64_t lo = h[mvk::IX_CTL_DG_NLO] ? ~h[mvk::IX_CTL_DG_NLO] : 0;
  const bool sweep = nb && h[mvk::IX_CTL_DG_NLO] && hi >= lo;  // else no leader has a record
  const uint64_t nbk = sweep ? hi - lo + 1 : 1;
  if (nbk > kMaxLinearBuckets) return set_err(ctx, MV_E_INVALID_ARG, "linearize: the leaders stand too many rounds above the store's lowest");

  mvk::LinState ls{};
  ls.mark = dg.lmark.as<uint32_t>();
  ls.n = n, ls.nbk = nbk, ls.lo = lo, ls.hi = hi;
  // control words; per leader: root_slot | first (u64) | fail | total (u32), behind the leaders of a host call
  HIPCHK(ctx, dg.lctl.ensure(8 * mvk::LN_CTL_WORDS));
  HIPCHK(ctx, hipMemsetAsync(dg.lctl.p, 0, 8 * mvk::LN_CTL_WORDS, s));
  ls.lctl = dg.lctl.as<uint64_t>();
  HIPCHK(ctx, hipMemsetAsync(ls.lctl + mvk::LN_CTL_LO, 0xff, 8, s));
  HIPCHK(ctx, dg.llead.ensure(ix_al(48 * n) + 2 * ix_al(8 * n) + 2 * ix_al(4 * n)));
  {
    char* b = dg.llead.as<char>();
    if (!d_leaders) {
      HIPCHK(ctx, hipMemcpyAsync(b, leaders, 48 * n, hipMemcpyHostToDevice, s));
      d_leaders = (const uint64_t*)b;
    }
    b += ix_al(48 * n);
    ls.leaders = d_leaders;
    ls.root_slot = (uint64_t*)b, ls.first = (uint64_t*)(b + ix_al(8 * n));
    ls.fail = (uint32_t*)(b + 2 * ix_al(8 * n)), ls.total = (uint32_t*)(b + 2 * ix_al(8 * n) + ix_al(4 * n));
  }
  const size_t best_bytes = 8 * (size_t)mvk::LN_KEY_WORDS * ix.slots;
  HIPCHK(ctx, dg.lbest.ensure(best_bytes));
  HIPCHK(ctx, hipMemsetAsync(dg.lbest.p, 0xff, best_bytes, s));
  ls.best = dg.lbest.as<uint64_t>();
  // per bucket: count (u32) | off (u64, one more) ; per level, and one more: lvl_start
  const size_t a_cnt = ix_al(4 * nbk), a_off = ix_al(8 * (nbk + 1)), a_lvl = ix_al(8 * (nbk + 2));
  HIPCHK(ctx, dg.lbk.ensure(a_cnt + a_off + a_lvl));
  ls.bk_count = dg.lbk.as<uint32_t>();
  uint64_t* d_off = (uint64_t*)(dg.lbk.as<char>() + a_cnt);
  ls.bk_off = d_off;
  ls.lvl_start = (uint64_t*)(dg.lbk.as<char>() + a_cnt + a_off);
  const mvk::IndexTable t = table_of(ctx, ix);
  const mvk::DagStore d = dag_view(dg);

  // the edges: counts per bucket, read back; their scan is the host's
  std::vector<uint32_t> count(nbk, 0);
  std::vector<uint64_t> off(nbk + 1, 0);
  if (sweep) {
    HIPCHK(ctx, hipMemsetAsync(ls.bk_count, 0, 4 * nbk, s));
    HIPCHK(ctx, mvk::launch_linear_edges(t, d, nb, ls, /*fill=*/false, ctl, s));
    HIPCHK(ctx, hipMemcpyAsync(count.data(), ls.bk_count, 4 * nbk, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (uint64_t b = 0; b < nbk; b++) off[b + 1] = off[b] + count[b];
  }
  const uint64_t n_edges = off[nbk];
  if (n_edges > dg.ni) return set_err(ctx, MV_E_HIP, "linearize: more edges than the store's includes");
  ls.n_edges = n_edges;
  ls.node_cap = sweep ? n_edges + n : 0;
  // the levels, downwards: a round that an edge ends in or a leader stands on; bucket 0 last
  std::vector<uint64_t> lv_round, lv_bucket;
  if (sweep) {
    std::vector<uint64_t> lr;
    for (size_t k = 0; k < n; k++)
      if (leaders[6 * k + 1] >= lo) lr.push_back(leaders[6 * k + 1]);
    std::sort(lr.begin(), lr.end());
    for (uint64_t b = nbk; b-- > 0;) {
      const uint64_t round = lo + b;  // bucket b + 1 (edges); rounds lo .. hi
      const bool led = std::binary_search(lr.begin(), lr.end(), round);
      const bool edges = b + 1 < nbk && count[b + 1];
      if (led || edges) lv_round.push_back(round), lv_bucket.push_back(b + 1 < nbk ? b + 1 : nbk);
    }
    if (count[0]) lv_round.push_back(~0ull), lv_bucket.push_back(0);
  }
  ls.n_levels = lv_round.size();
  if (sweep) {
    HIPCHK(ctx, hipMemcpyAsync(d_off, off.data(), 8 * (nbk + 1), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemsetAsync(ls.bk_count, 0, 4 * nbk, s));
    HIPCHK(ctx, dg.ledge.ensure(sizeof(mvk::LinEdge) * (size_t)n_edges + 16));
    ls.edges = dg.ledge.as<mvk::LinEdge>();
    // per node: slot | round | path x 4 (u64) | cidx | depth | t | lvl (u32); per record: node_of_rec
    const size_t nc = ls.node_cap, a8 = ix_al(8 * nc), a4 = ix_al(4 * nc);
    HIPCHK(ctx, dg.lnode.ensure(6 * a8 + 4 * a4 + ix_al(4 * nb) + ix_al(8 * nb)));
    char* b = dg.lnode.as<char>();
    ls.n_slot = (uint64_t*)b, ls.n_round = (uint64_t*)(b + a8), ls.n_path = (uint64_t*)(b + 2 * a8);
    b += 2 * a8 + mvk::LN_PATH_WORDS * a8;
    ls.n_cidx = (uint32_t*)b, ls.n_depth = (uint32_t*)(b + a4), ls.n_t = (uint32_t*)(b + 2 * a4), ls.n_lvl = (uint32_t*)(b + 3 * a4);
    ls.node_of_rec = (uint32_t*)(b + 4 * a4);
    ls.rec_low = (uint64_t*)(b + 4 * a4 + ix_al(4 * nb));
    HIPCHK(ctx, hipMemsetAsync(ls.node_of_rec, 0xff, 4 * (size_t)nb, s));
    HIPCHK(ctx, mvk::launch_linear_edges(t, d, nb, ls, /*fill=*/true, ctl, s));
  }
  if (!d_blocks) {
    const uint64_t rows = std::min<uint64_t>(cap, ls.node_cap);
    HIPCHK(ctx, dg.lres.ensure(48 * (size_t)rows + 16));
    d_blocks = dg.lres.as<uint64_t>();
    cap = rows;
    if (own_blocks) *own_blocks = d_blocks;
  }
  HIPCHK(ctx, mvk::launch_linear_roots(t, d, nb, ls, ctl, s));
  // The levels in growing runs, with the lowest round the nodes so far can reach read back behind each:
  // a level has work only at or above it, or where a leader still stands at or below the level. Nodes are
  // made by the levels alone, so once neither holds for a level it holds for none behind it.
  uint64_t lowest_leader = ~0ull;
  for (size_t k = 0; k < n; k++)
    if (leaders[6 * k + 1] >= lo) lowest_leader = std::min(lowest_leader, leaders[6 * k + 1]);
  size_t l = 0;
  for (size_t run = 4; l < lv_round.size(); run = std::min<size_t>(2 * run, 64)) {
    uint64_t low = ~0ull;
    if (l) {
      HIPCHK(ctx, hipMemcpyAsync(&low, ls.lctl + mvk::LN_CTL_LO, 8, hipMemcpyDeviceToHost, s));
      HIPCHK(ctx, hipStreamSynchronize(s));
    }
    const uint64_t round = lv_round[l];  // all ones: bucket 0, the rounds below lo
    const bool led = round != ~0ull && lowest_leader <= round;
    const bool reached = low != ~0ull && (round == ~0ull ? low < lo : low <= round);
    if (!led && !reached) break;
    for (const size_t end = std::min(l + run, lv_round.size()); l < end; l++) {
      const uint64_t b = lv_bucket[l];
      const uint64_t e0 = b < nbk ? off[b] : 0, ne = b < nbk ? count[b] : 0;  // (the highest leader round has no bucket)
      HIPCHK(ctx, mvk::launch_linear_level(t, d, nb, ls, l, lv_round[l], e0, ne, ctl, s));
    }
  }
  ls.n_levels = l;  // the levels that ran: the output step closes the last one's nodes
  HIPCHK(ctx, mvk::launch_linear_output(t, ls, dg.lin_height, cap, d_sub, d_blocks, ctl, s));
  uint64_t w[mvk::LN_CTL_WORDS];
  HIPCHK(ctx, hipMemcpyAsync(w, ls.lctl, sizeof(w), hipMemcpyDeviceToHost, s));
  st = read_ctl(ctx, dev, s, nullptr);  // (synchronises)
  if (st != MV_OK) return st;
  dg.lin_height += std::min<uint64_t>(w[mvk::LN_CTL_NOK], n);
  dg.lin_marked += std::min<uint64_t>(w[mvk::LN_CTL_NEWMARK], ls.node_cap);
  *n_rows = std::min<uint64_t>(w[mvk::LN_CTL_NROWS], cap);
  return MV_OK;
}
}  // namespace

mv_status mvi::linear_marks_for(mv_ctx* ctx, Device& dev, uint64_t old_slots, const mvk::IndexTable& nt, uint64_t slots,
                                DevBuf& fresh, hipStream_t s) {
  Index& ix = dev.index;
  if (fresh.ensure(4 * (size_t)slots) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "no device memory for the linearizer's marks");
  }
  HIPCHK(ctx, hipMemsetAsync(fresh.p, 0, 4 * (size_t)slots, s));
  if (old_slots && ix.dag.lmark.p && ix.dag.lin_marked)
    HIPCHK(ctx, mvk::launch_linear_carry(ix.tab.as<uint64_t>(), old_slots, ix.dag.lmark.as<uint32_t>(), nt, fresh.as<uint32_t>(),
                                         ix.ctl.as<uint64_t>(), s));
  return MV_OK;
}

extern "C" {

mv_status mv_linearize(mv_ctx* ctx, const uint64_t* leaders, uint32_t n, uint64_t* blocks, uint64_t cap, uint64_t* sub,
                       uint64_t* n_rows) {
  if (!ctx || !n_rows || (n && (!leaders || !sub)) || (cap && !blocks)) return set_err(ctx, MV_E_INVALID_ARG, "bad linearize args");
  *n_rows = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Dag& dg = dev->index.dag;
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n > MV_LINEAR_MAX_LEADERS) return set_err(ctx, MV_E_INVALID_ARG, "linearize: more than MV_LINEAR_MAX_LEADERS leaders");
  if (n == 0) return MV_OK;
  hipStream_t s = dev->stream;
  // (the sub rows stand in a buffer of their own: the blocks' buffer is made inside the call)
  HIPCHK(ctx, dg.res.ensure(32 * (size_t)n));
  uint64_t* d_sub = dg.res.as<uint64_t>();
  uint64_t* d_blocks = nullptr;
  st = linearize_run(ctx, *dev, leaders, nullptr, n, nullptr, cap, d_sub, s, n_rows, &d_blocks);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(sub, d_sub, 32 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (*n_rows && d_blocks) HIPCHK(ctx, hipMemcpyAsync(blocks, d_blocks, 48 * (size_t)*n_rows, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return MV_OK;
}

mv_status mv_dev_linearize(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_blocks, uint64_t cap,
                           uint64_t* d_sub, uint64_t* n_rows, void* stream) {
  if (!ctx || !n_rows || (n && (!d_leaders || !d_sub)) || (cap && !d_blocks))
    return set_err(ctx, MV_E_INVALID_ARG, "bad linearize args");
  *n_rows = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  if (!dev->index.dag.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n > MV_LINEAR_MAX_LEADERS) return set_err(ctx, MV_E_INVALID_ARG, "linearize: more than MV_LINEAR_MAX_LEADERS leaders");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  std::vector<uint64_t> leaders(6 * (size_t)n);  // their rounds choose the levels, on the host
  HIPCHK(ctx, hipMemcpyAsync(leaders.data(), d_leaders, 48 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  // (cap == 0: a one-row buffer of the context's stands in, and nothing is written to it)
  uint64_t* own = nullptr;
  st = linearize_run(ctx, *dev, leaders.data(), d_leaders, n, cap ? d_blocks : nullptr, cap, d_sub, s, n_rows, &own);
  if (st != MV_OK) (void)hipStreamSynchronize(s);
  return st;
}

mv_status mv_linearize_mark(mv_ctx* ctx, const uint64_t* refs, uint64_t n, uint64_t height) {
  if (!ctx || (n && !refs) || n > mvk::IX_MAX_ITEMS) return set_err(ctx, MV_E_INVALID_ARG, "bad linearize_mark args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  Dag& dg = ix.dag;
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  hipStream_t s = dev->stream;
  if (n) {
    st = index_room_for_more(ctx, *dev, n, /*can_grow=*/true, s);
    if (st != MV_OK) return st;
    if (!dg.lmark.p || dg.map_slots != ix.slots) return set_err(ctx, MV_E_HIP, "the linearizer's marks do not match the index");
    HIPCHK(ctx, ix.keys.ensure(48 * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(ix.keys.p, refs, 48 * (size_t)n, hipMemcpyHostToDevice, s));
    st = insert_rounds(ctx, *dev, mvk::IndexKeys{ix.keys.as<uint8_t>(), nullptr, 48, 0}, n, MV_REF_STORED, s);
    if (st != MV_OK) return st;
    HIPCHK(ctx, dg.lctl.ensure(8 * mvk::LN_CTL_WORDS));
    HIPCHK(ctx, hipMemsetAsync(dg.lctl.p, 0, 8 * mvk::LN_CTL_WORDS, s));
    HIPCHK(ctx, mvk::launch_linear_mark(ix.item.as<uint64_t>(), n, dg.lmark.as<uint32_t>(), ix.slots, dg.lctl.as<uint64_t>(),
                                        ix.ctl.as<uint64_t>(), s));
    uint64_t w[mvk::LN_CTL_WORDS];
    HIPCHK(ctx, hipMemcpyAsync(w, dg.lctl.p, sizeof(w), hipMemcpyDeviceToHost, s));
    st = read_ctl(ctx, *dev, s, nullptr);
    if (st != MV_OK) return st;
    dg.lin_marked += std::min<uint64_t>(w[mvk::LN_CTL_NEWMARK], n);
  }
  dg.lin_height = std::max(dg.lin_height, height);
  return MV_OK;
}

mv_status mv_linearize_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad linearize_stats args");
  out[0] = out[1] = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  out[0] = dev->index.dag.lin_marked, out[1] = dev->index.dag.lin_height;
  return MV_OK;
}

}  // extern "C"
