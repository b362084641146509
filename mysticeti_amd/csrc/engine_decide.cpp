// libmysti_verify.so: the decision rules over the DAG store (mv_decide_leaders,
// mv_commit_leaders): the host side of decide.hip.
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

using namespace mvi;

namespace {
constexpr uint64_t kMaxDecideWaves = 1ull << 26;

// One decide call on stream s (include/mysti_verify.h, mv_decide_leaders): the rows sorted by round
// on the host, the PickRoles pass, the counts of voting and decision records read back (they size the
// next launches), k_dg_vote, k_dg_cert, k_dg_decide. Results go to d_out / d_stakes (device).
// A commit call passes `keep`: k_dg_cert then also leaves its certificate masks, and the call's
// arrays are handed on; without it the launches are those of a decide call, one for one.
struct DecideKeep {
  mvk::DecideIn in;
  mvk::DecideState ds;
  uint64_t nvote, ndec;
};
mv_status decide_run(mv_ctx* ctx, Device& dev, const uint64_t* leaders, uint32_t n32, uint64_t* d_out, uint64_t* d_stakes,
                     hipStream_t s, DecideKeep* keep = nullptr) {
  Index& ix = dev.index;
  Dag& dg = ix.dag;
  const size_t n = n32;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return leaders[2 * x + 1] < leaders[2 * y + 1]; });
  // g_round (ng) | g_start (ng + 1) | l_auth | l_round | l_row (n each): laid out for ng = n, the most
  std::vector<uint64_t> tab(5 * n + 1);
  uint64_t *g_round = tab.data(), *g_start = g_round + n, *l_auth = g_start + n + 1, *l_round = l_auth + n, *l_row = l_round + n;
  uint64_t ng = 0, gmax = 1;
  for (size_t k = 0; k < n; k++) {
    const uint64_t a = leaders[2 * (size_t)order[k]], r = leaders[2 * (size_t)order[k] + 1];
    l_auth[k] = a, l_round[k] = r, l_row[k] = order[k];
    if (ng == 0 || g_round[ng - 1] != r) g_round[ng] = r, g_start[ng] = k, ng++;
    gmax = std::max<uint64_t>(gmax, k + 1 - g_start[ng - 1]);
  }
  g_start[ng] = n;
  HIPCHK(ctx, dg.lead.ensure(8 * tab.size()));
  HIPCHK(ctx, hipMemcpyAsync(dg.lead.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, s));
  const uint64_t* dl = dg.lead.as<uint64_t>();
  const mvk::DecideIn in{dl, dl + n, dl + 2 * n + 1, dl + 3 * n + 1, dl + 4 * n + 1, ng, n, gmax};
  // per row: cand_slot (8 u64) | blame (16 u32) | vote (8 x 16) | cert (8 x 16) | cand_n
  const size_t state_bytes = (64 + 4 * (size_t)(mvk::DG_BM_WORDS * 17 + 1)) * n;
  HIPCHK(ctx, dg.state.ensure(state_bytes));
  HIPCHK(ctx, hipMemsetAsync(dg.state.p, 0, state_bytes, s));
  const uint64_t nb = dg.nb;
  HIPCHK(ctx, dg.lists.ensure(12 * (size_t)nb + 4));
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(nb) + 8));
  mvk::DecideState ds{};
  ds.cand_slot = dg.state.as<uint64_t>();
  ds.blame = (uint32_t*)(ds.cand_slot + 8 * n);
  ds.vote = ds.blame + mvk::DG_BM_WORDS * n;
  ds.cert = ds.vote + 8 * mvk::DG_BM_WORDS * n;
  ds.cand_n = ds.cert + 8 * mvk::DG_BM_WORDS * n;
  ds.vpos = dg.lists.as<uint32_t>(), ds.vlist = ds.vpos + nb, ds.dlist = ds.vlist + nb;
  const mvk::DagStore d = dag_view(dg);
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_DG_NVOTE, 0, 16, s));
  HIPCHK(ctx, mvk::launch_decide_pick(d, nb, in, ds, ix.wg.as<uint64_t>(), ctl, s));
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  const uint64_t nvote = std::min<uint64_t>(h[mvk::IX_CTL_DG_NVOTE], nb), ndec = std::min<uint64_t>(h[mvk::IX_CTL_DG_NDEC], nb);
  if (nvote * gmax > kMaxDecideWaves || ndec * gmax > kMaxDecideWaves)
    return set_err(ctx, MV_E_INVALID_ARG, "decide: too many leader rows of one round for the records of its rounds");
  HIPCHK(ctx, dg.sup.ensure(8 * (size_t)(nvote * gmax) + 8));
  ds.sup = dg.sup.as<uint64_t>();
  if (keep) {
    HIPCHK(ctx, dg.cmask.ensure((size_t)(ndec * gmax) + 8));
    HIPCHK(ctx, hipMemsetAsync(dg.cmask.p, 0, (size_t)(ndec * gmax) + 8, s));
    ds.cmask = dg.cmask.as<uint8_t>();
  }
  const auto& com = ctx->committee;
  HIPCHK(ctx, mvk::launch_decide_rule(table_of(ctx, ix), d, nb, in, ds, nvote, ndec, dev.tab.stakes.as<uint64_t>(), com.size(),
                                      com.quorum_threshold, d_out, d_stakes, ctl, s));
  if (keep) *keep = DecideKeep{in, ds, nvote, ndec};
  return MV_OK;
}

// One commit call on stream s (include/mysti_verify.h, mv_commit_leaders): the direct stages, then
// passes of chain step -> reach -> resolve while a pass moves a row (each pass reads its control
// words back: the jobs and their levels size the next launches), then the prefix. Every pass ends
// at least the highest row that is not final, so there are at most n of them. Results go to d_out /
// d_info (device); the caller reads ctl[IX_CTL_CM_NSEQ] back.
mv_status commit_run(mv_ctx* ctx, Device& dev, const uint64_t* leaders, uint32_t n32, uint64_t* d_out, uint64_t* d_info,
                     hipStream_t s) {
  Index& ix = dev.index;
  Dag& dg = ix.dag;
  const size_t n = n32;
  for (size_t i = 1; i < n; i++)
    if (leaders[2 * i + 1] < leaders[2 * i - 1])
      return set_err(ctx, MV_E_INVALID_ARG, "commit: the leader rows are not in non-decreasing round order");
  DecideKeep k{};
  mv_status st = decide_run(ctx, dev, leaders, n32, d_out, nullptr, s, &k);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  const uint64_t nb = dg.nb;
  // per row: cslot | job_low | job_miss (u64 each) | fin | act | anchor | job_id | jobs (u32 each)
  HIPCHK(ctx, dg.cm.ensure(44 * n));
  mvk::CommitState cs{};
  cs.cslot = dg.cm.as<uint64_t>(), cs.job_low = cs.cslot + n, cs.job_miss = cs.job_low + n;
  cs.fin = (uint32_t*)(cs.job_miss + n), cs.act = cs.fin + n, cs.anchor = cs.act + n, cs.job_id = cs.anchor + n;
  cs.jobs = cs.job_id + n;
  cs.mark_words = (nb + 31) / 32;
  const mvk::IndexTable t = table_of(ctx, ix);
  const mvk::DagStore d = dag_view(dg);
  HIPCHK(ctx, mvk::launch_commit_init(t, k.in, k.ds, cs, d_out, d_info, ctl, s));
  // a level q reads the records of round q + 1, r + 3 <= q + 1 <= R: the rounds between the rows' ends
  HIPCHK(ctx, dg.span.ensure(4 * (size_t)nb + 4));
  cs.span = dg.span.as<uint32_t>();
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_CM_NSPAN, 0, 8, s));
  if (leaders[1] <= ~0ull - 3)
    HIPCHK(ctx, mvk::launch_commit_span(d, nb, leaders[1] + 3, leaders[2 * n - 1], cs.span, ix.wg.as<uint64_t>(), ctl, s));
  std::vector<uint32_t> h_act(2 * n);
  std::vector<uint64_t> levels;
  for (size_t pass = 0; pass <= n; pass++) {
    HIPCHK(ctx, hipMemsetAsync(cs.job_low, 0xff, 8 * n, s));
    HIPCHK(ctx, hipMemsetAsync(cs.job_miss, 0, 8 * n, s));
    HIPCHK(ctx, hipMemsetAsync(cs.job_id, 0xff, 4 * n, s));
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_CM_NJOBS, 0, 8 * 4, s));
    HIPCHK(ctx, mvk::launch_commit_chain(k.in, cs, d_out, ctl, s));
    const uint64_t* h = nullptr;
    st = read_ctl(ctx, dev, s, &h);
    if (st != MV_OK) return st;
    if (h[mvk::IX_CTL_CM_MOVED] == 0) break;
    const uint64_t njobs = h[mvk::IX_CTL_DG_NLO] ? std::min<uint64_t>(h[mvk::IX_CTL_CM_NJOBS], n) : 0;
    if (njobs) {
      // the levels some walk passes, inside the store's rounds (outside them there is no record): act | anchor
      // come back, and the rows' rounds are the host's
      const uint64_t qhi = std::min<uint64_t>(h[mvk::IX_CTL_CM_QHI], h[mvk::IX_CTL_DG_HI]);
      const uint64_t qlo = std::max<uint64_t>(~h[mvk::IX_CTL_CM_NQLO], ~h[mvk::IX_CTL_DG_NLO]);
      const uint64_t nspan = std::min<uint64_t>(h[mvk::IX_CTL_CM_NSPAN], nb);
      HIPCHK(ctx, hipMemcpyAsync(h_act.data(), cs.act, 8 * n, hipMemcpyDeviceToHost, s));
      HIPCHK(ctx, hipStreamSynchronize(s));
      levels.clear();
      if (qhi > qlo && qhi - qlo > (1ull << 24)) return set_err(ctx, MV_E_INVALID_ARG, "commit: a walk spans too many rounds");
      if (qhi > qlo) {
        std::vector<uint8_t> on(qhi - qlo, 0);
        for (size_t i = 0; i < n; i++) {
          const uint64_t j = h_act[n + i];
          if (h_act[i] != mvk::CM_ACT_WALK || j >= n) continue;
          const uint64_t lo = std::max<uint64_t>(leaders[2 * i + 1] + 2, qlo), hi = std::min<uint64_t>(leaders[2 * j + 1], qhi);
          for (uint64_t q = lo; q < hi; q++) on[q - qlo] = 1;
        }
        for (uint64_t q = qhi; q > qlo; q--)
          if (on[q - 1 - qlo]) levels.push_back(q - 1);
      }
      if (njobs * cs.mark_words > (1ull << 32)) return set_err(ctx, MV_E_INVALID_ARG, "commit: too many walks for the store's records");
      HIPCHK(ctx, dg.marks.ensure(4 * (size_t)(njobs * cs.mark_words) + 4));
      HIPCHK(ctx, hipMemsetAsync(dg.marks.p, 0, 4 * (size_t)(njobs * cs.mark_words) + 4, s));
      cs.marks = dg.marks.as<uint32_t>();
      HIPCHK(ctx, mvk::launch_commit_reach(t, d, nb, k.in, cs, njobs, nspan, levels.data(), levels.size(), ctl, s));
    }
    HIPCHK(ctx, mvk::launch_commit_resolve(t, d, nb, k.in, k.ds, cs, k.nvote, k.ndec, njobs, d_out, d_info, ctl, s));
  }
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_CM_NSEQ, 0, 8, s));
  HIPCHK(ctx, mvk::launch_commit_prefix(k.in, d_out, ctl, s));
  return MV_OK;
}
}  // namespace

extern "C" {

mv_status mv_decide_leaders(mv_ctx* ctx, const uint64_t* leaders, uint32_t n, uint64_t* out, uint64_t* stakes) {
  if (!ctx || (n && (!leaders || !out))) return set_err(ctx, MV_E_INVALID_ARG, "bad decide args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Dag& dg = dev->index.dag;
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n == 0) return MV_OK;
  hipStream_t s = dev->stream;
  const size_t nn = n;
  HIPCHK(ctx, dg.res.ensure(8 * 11 * nn));
  uint64_t* d_out = dg.res.as<uint64_t>();
  st = decide_run(ctx, *dev, leaders, n, d_out, stakes ? d_out + 8 * nn : nullptr, s);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(out, d_out, 64 * nn, hipMemcpyDeviceToHost, s));
  if (stakes) HIPCHK(ctx, hipMemcpyAsync(stakes, d_out + 8 * nn, 24 * nn, hipMemcpyDeviceToHost, s));
  return read_ctl(ctx, *dev, s, nullptr);
}

mv_status mv_commit_leaders(mv_ctx* ctx, const uint64_t* leaders, uint32_t n, uint64_t* out, uint64_t* info,
                            uint64_t* n_sequence) {
  if (!ctx || !n_sequence || (n && (!leaders || !out || !info))) return set_err(ctx, MV_E_INVALID_ARG, "bad commit args");
  *n_sequence = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Dag& dg = dev->index.dag;
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n == 0) return MV_OK;
  hipStream_t s = dev->stream;
  const size_t nn = n;
  HIPCHK(ctx, dg.res.ensure(8 * 12 * nn));
  uint64_t* d_out = dg.res.as<uint64_t>();
  st = commit_run(ctx, *dev, leaders, n, d_out, d_out + 8 * nn, s);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(out, d_out, 64 * nn, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(info, d_out + 8 * nn, 32 * nn, hipMemcpyDeviceToHost, s));
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, *dev, s, &h);
  if (st == MV_OK) *n_sequence = std::min<uint64_t>(h[mvk::IX_CTL_CM_NSEQ], n);
  return st;
}

mv_status mv_dev_commit_leaders(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_out,
                                uint64_t* d_info, uint64_t* n_sequence, void* stream) {
  if (!ctx || !n_sequence || (n && (!d_leaders || !d_out || !d_info))) return set_err(ctx, MV_E_INVALID_ARG, "bad commit args");
  *n_sequence = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  if (!dev->index.dag.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  std::vector<uint64_t> leaders(2 * (size_t)n);  // their order is checked, and the rounds grouped, on the host
  HIPCHK(ctx, hipMemcpyAsync(leaders.data(), d_leaders, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  st = commit_run(ctx, *dev, leaders.data(), n, d_out, d_info, s);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, *dev, s, &h);
  if (st == MV_OK) *n_sequence = std::min<uint64_t>(h[mvk::IX_CTL_CM_NSEQ], n);
  return st;
}

mv_status mv_dev_decide_leaders(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_out,
                                uint64_t* d_stakes, void* stream) {
  if (!ctx || (n && (!d_leaders || !d_out))) return set_err(ctx, MV_E_INVALID_ARG, "bad decide args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  if (!dev->index.dag.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  std::vector<uint64_t> leaders(2 * (size_t)n);  // sorted by round on the host
  HIPCHK(ctx, hipMemcpyAsync(leaders.data(), d_leaders, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  st = decide_run(ctx, *dev, leaders.data(), n, d_out, d_stakes, s);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  return read_ctl(ctx, *dev, s, nullptr);
}

}  // extern "C"
