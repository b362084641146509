// libmysti_verify.so: the suspended-block store and the connect call (mv_pending_*,
// mv_connect_blocks): the host side of pending.hip, on top of the accept call (engine_index.cpp).
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

using namespace mvi;

// copy k of the suspended-block store as the kernels see it
mvk::PendStore mvi::pend_view(const Pending& pd, int k) {
  char* b = pd.blk[k].as<char>();
  return mvk::PendStore{(uint64_t*)b, (uint64_t*)(b + 8 * pd.cap_b), (uint64_t*)(b + 16 * pd.cap_b),
                        (uint32_t*)(b + 24 * pd.cap_b), pd.inc[k].as<uint64_t>()};
}

// Room in the suspended-block store for more_b blocks and more_i includes on top of those there.
// Growing keeps the records of the copy in force. Synchronises s when it grows.
mv_status mvi::pending_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, bool can_grow, hipStream_t s) {
  Pending& pd = dev.index.pend;
  const uint64_t need_b = pd.nb + more_b, need_i = pd.ni + more_i;
  if (need_b <= pd.cap_b && need_i <= pd.cap_i) return MV_OK;
  if (!can_grow)
    return set_err(ctx, MV_E_INDEX_FULL,
                   "suspended-block store: " + std::to_string(pd.nb) + " blocks + " + std::to_string(more_b) + " and " +
                       std::to_string(pd.ni) + " includes + " + std::to_string(more_i) + " that the call may add > " +
                       std::to_string(pd.cap_b) + " and " + std::to_string(pd.cap_i) + " reserved (mv_pending_reserve)");
  if (need_b > mvk::IX_MAX_ITEMS || need_i > (1ull << 40)) return set_err(ctx, MV_E_INVALID_ARG, "too many suspended blocks");
  Pending fresh;
  fresh.cap_b = need_b > pd.cap_b ? std::max<uint64_t>(need_b, 2 * pd.cap_b) : pd.cap_b;
  fresh.cap_i = need_i > pd.cap_i ? std::max<uint64_t>(need_i, 2 * pd.cap_i) : pd.cap_i;
  for (int k = 0; k < 2; k++)
    if (fresh.blk[k].ensure(28 * (size_t)fresh.cap_b) != hipSuccess || fresh.inc[k].ensure(8 * (size_t)fresh.cap_i) != hipSuccess) {
      (void)hipGetLastError();
      return set_err(ctx, MV_E_ALLOC, "no device memory for the suspended-block store");
    }
  if (pd.nb) {
    const mvk::PendStore from = pend_view(pd, pd.cur), to = pend_view(fresh, 0);
    HIPCHK(ctx, hipMemcpyAsync(to.slot, from.slot, 8 * (size_t)pd.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.ibase, from.ibase, 8 * (size_t)pd.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.blk, from.blk, 8 * (size_t)pd.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.kc, from.kc, 4 * (size_t)pd.nb, hipMemcpyDeviceToDevice, s));
    if (pd.ni) HIPCHK(ctx, hipMemcpyAsync(to.inc, from.inc, 8 * (size_t)pd.ni, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));  // the old copies are read until here; `fresh` frees them below
  for (int k = 0; k < 2; k++) {
    std::swap(pd.blk[k], fresh.blk[k]);
    std::swap(pd.inc[k], fresh.inc[k]);
  }
  pd.cur = 0;
  pd.cap_b = fresh.cap_b, pd.cap_i = fresh.cap_i;
  return MV_OK;
}

namespace {
// Step 6 of a connect call on stream s, after accept_run (or alone: n = 0): the NEW blocks join the
// store, the sweep, the compaction. Rows go to d_rows (cap rows; the caller's device memory, or
// pend.rows). Synchronises s: the appended counts, the level counts of every few levels enqueued
// together, and what the compaction kept are read back.
mv_status connect_sweep(mv_ctx* ctx, Device& dev, const AcceptOut& ao, uint64_t* d_rows, uint64_t cap, hipStream_t s,
                        uint64_t* n_connected) {
  Index& ix = dev.index;
  Pending& pd = ix.pend;
  *n_connected = 0;
  pd.levels = 0;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  const uint64_t* h = nullptr;
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_PB_NB, 0, 8 * (mvk::IX_CTL_PB_END - mvk::IX_CTL_PB_NB), s));
  if (ao.ncand) {  // (accept_run made room for ncand blocks and ninc includes)
    HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(ao.ncand)));
    HIPCHK(ctx, pd.cand_dst.ensure(8 * (size_t)ao.ncand));
    HIPCHK(ctx, mvk::launch_pend_append(ao.a, ao.ncand, ao.ninc, ix.item.as<uint64_t>(), pd.cand_slot.as<uint64_t>(),
                                        pd.cand_dst.as<uint64_t>(), pend_view(pd, pd.cur), pd.nb, pd.ni,
                                        ix.wg.as<uint64_t>(), ctl, s));
    st = read_ctl(ctx, dev, s, &h);
    if (st != MV_OK) return st;
    pd.nb += std::min<uint64_t>(h[mvk::IX_CTL_PB_NB], ao.ncand);
    pd.ni += std::min<uint64_t>(h[mvk::IX_CTL_PB_NI], ao.ninc);
  }
  const uint64_t nb = pd.nb;
  if (nb == 0) return MV_OK;
  const mvk::IndexTable t = table_of(ctx, ix);
  const mvk::PendStore p = pend_view(pd, pd.cur), q = pend_view(pd, pd.cur ^ 1);
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(nb)));
  HIPCHK(ctx, pd.lvl.ensure(4 * (size_t)nb));
  HIPCHK(ctx, pd.hit.ensure((size_t)nb));
  HIPCHK(ctx, pd.newbase.ensure(8 * (size_t)nb));
  HIPCHK(ctx, hipMemsetAsync(pd.lvl.p, 0, 4 * (size_t)nb, s));
  Dag& dg = ix.dag;
  if (dg.on) HIPCHK(ctx, pd.row_of.ensure(4 * (size_t)nb));
  uint32_t* row_of = dg.on ? pd.row_of.as<uint32_t>() : nullptr;
  // the sweep: levels are enqueued 2, 4, 8, then 16 at a time and their counts read together; a
  // level past the fixed point lists nothing. At most nb levels connect something.
  uint64_t level = 0;
  for (int ahead = 2;; ahead = std::min(2 * ahead, mvk::IX_CTL_LEVELS)) {
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_LV0, 0, 8 * mvk::IX_CTL_LEVELS, s));
    const int m = (int)std::min<uint64_t>(ahead, nb + 1 - level);
    for (int k = 0; k < m; k++)
      HIPCHK(ctx, mvk::launch_pend_level(t, p, nb, pd.lvl.as<uint32_t>(), pd.hit.as<uint8_t>(), level + k,
                                         ix.wg.as<uint64_t>(), d_rows, cap, ctl, mvk::IX_CTL_LV0 + k, row_of, s));
    st = read_ctl(ctx, dev, s, &h);
    if (st != MV_OK) return st;
    int k = 0;
    while (k < m && h[mvk::IX_CTL_LV0 + k]) k++;
    level += k;
    if (k < m) break;
    if (level > nb) return set_err(ctx, MV_E_HIP, "connect: the sweep did not reach its fixed point");
  }
  pd.levels = level;
  *n_connected = h[mvk::IX_CTL_PB_ROWS];
  // with a DAG store: the rows' records join it, in row order, before the compaction drops them
  // (the includes they bring are at most those the suspended-block store holds)
  const uint64_t dag_rows = dg.on ? std::min<uint64_t>(h[mvk::IX_CTL_PB_ROWS], nb) : 0, dag_ni_cap = pd.ni;
  if (dag_rows) {
    st = dag_room(ctx, dev, dag_rows, pd.ni, s);
    if (st != MV_OK) return st;
    HIPCHK(ctx, dg.src.ensure(8 * (size_t)dag_rows));
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_DG_NI, 0, 8, s));
    HIPCHK(ctx, mvk::launch_dag_append(t, p, nb, pd.lvl.as<uint32_t>(), row_of, dag_rows, dag_view(dg), dg.nb, dg.ni,
                                       dg.src.as<uint64_t>(), ix.wg.as<uint64_t>(), ctl, s));
  }
  // what stays is blocks_pending
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_PB_NB, 0, 16, s));
  HIPCHK(ctx, mvk::launch_pend_compact(t, p, q, nb, pd.newbase.as<uint64_t>(), ao.a.state, ao.a.n, ix.wg.as<uint64_t>(), ctl, s));
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  pd.nb = std::min<uint64_t>(h[mvk::IX_CTL_PB_NB], nb);
  pd.ni = std::min<uint64_t>(h[mvk::IX_CTL_PB_NI], pd.ni);
  pd.cur ^= 1;
  if (dag_rows) {
    dg.nb += dag_rows;
    dg.ni += std::min<uint64_t>(h[mvk::IX_CTL_DG_NI], dag_ni_cap);
  }
  return MV_OK;
}
}  // namespace

extern "C" {

mv_status mv_pending_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t includes) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  const Pending& pd = dev->index.pend;
  return pending_room(ctx, *dev, blocks > pd.nb ? blocks - pd.nb : 0, includes > pd.ni ? includes - pd.ni : 0,
                      /*can_grow=*/true, dev->stream);
}

mv_status mv_pending_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad pending_stats args");
  memset(out, 0, 4 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  out[1] = ix.pend.nb, out[2] = ix.pend.ni, out[3] = ix.pend.levels;
  if (!ix.ctl.p) return MV_OK;
  const uint64_t* w = nullptr;
  st = read_ctl(ctx, *dev, dev->stream, &w);
  out[0] = w ? w[mvk::IX_CTL_STORED] : 0;
  return st;
}

mv_status mv_connect_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, const uint64_t* grp,
                            uint32_t n, uint8_t* blk_status, uint8_t* blk_state, uint64_t* missing, uint64_t cap_missing,
                            uint64_t* n_missing, uint64_t* connected, uint64_t cap_connected, uint64_t* n_connected) {
  if (!ctx || !n_missing || !n_connected || (n && (!buf || !off || !len || !blk_status || !blk_state)) ||
      (cap_missing && !missing) || (cap_connected && !connected))
    return set_err(ctx, MV_E_INVALID_ARG, "bad connect args");
  *n_missing = *n_connected = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  hipStream_t s = dev->stream;
  AcceptOut ao;
  const size_t nn = n;
  if (n) {
    st = stage_blocks(ctx, *dev, buf, off, len, grp, n, cap_missing, s, ao, /*connect=*/true);
    if (st != MV_OK) {
      (void)hipStreamSynchronize(s);  // (the copies may still be in flight)
      return st;
    }
  }
  // the rows: at most the records the store holds once this call's blocks joined it
  const uint64_t capd = std::min<uint64_t>(cap_connected, ix.pend.nb + ao.ncand);
  HIPCHK(ctx, ix.pend.rows.ensure(64 * (size_t)capd + 8));
  uint64_t total = 0;
  st = connect_sweep(ctx, *dev, ao, ix.pend.rows.as<uint64_t>(), capd, s, &total);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(blk_status, ao.status, nn, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(blk_state, ao.state, nn, hipMemcpyDeviceToHost, s));
  }
  const uint64_t wr = std::min(ao.n_missing, cap_missing), wc = std::min(total, capd);
  if (wr) HIPCHK(ctx, hipMemcpyAsync(missing, ao.missing, 48 * (size_t)wr, hipMemcpyDeviceToHost, s));
  if (wc) HIPCHK(ctx, hipMemcpyAsync(connected, ix.pend.rows.p, 64 * (size_t)wc, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *n_missing = ao.n_missing;
  *n_connected = total;
  return MV_OK;
}

mv_status mv_dev_connect_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                                const uint64_t* d_len, const uint64_t* d_grp, uint32_t n, uint8_t* d_blk_status,
                                uint8_t* d_blk_state, uint64_t* d_missing, uint64_t cap_missing, uint64_t* n_missing,
                                uint64_t* d_connected, uint64_t cap_connected, uint64_t* n_connected, void* stream) {
  if (!ctx || !n_missing || !n_connected || (n && (!d_buf || !d_off || !d_len || !d_blk_status || !d_blk_state)) ||
      (cap_missing && !d_missing) || (cap_connected && !d_connected))
    return set_err(ctx, MV_E_INVALID_ARG, "bad connect args");
  if (((uintptr_t)d_buf) & 7) return set_err(ctx, MV_E_INVALID_ARG, "d_buf must be 8-byte aligned");
  *n_missing = *n_connected = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  AcceptOut ao;
  if (n) st = accept_run(ctx, *dev, d_buf, buf_bytes, d_off, d_len, d_grp, n, cap_missing, /*can_grow=*/false, s, ao,
                         /*connect=*/true);
  uint64_t total = 0;
  if (st == MV_OK) st = connect_sweep(ctx, *dev, ao, d_connected, cap_connected, s, &total);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(d_blk_status, ao.status, (size_t)n, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_blk_state, ao.state, (size_t)n, hipMemcpyDeviceToDevice, s));
  }
  const uint64_t wr = std::min(ao.n_missing, cap_missing);
  if (wr) HIPCHK(ctx, hipMemcpyAsync(d_missing, ao.missing, 48 * (size_t)wr, hipMemcpyDeviceToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *n_missing = ao.n_missing;
  *n_connected = total;
  return MV_OK;
}

}  // extern "C"
