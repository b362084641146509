// libmysti_verify.so: the DAG store (mv_dag_reserve, mv_dag_stats, mv_dag_prune) and its seeding
// from a replayed WAL (mv_dev_dag_seed_rows): the host side of dag_store.hip.
#include <string.h>

#include <algorithm>

#include "engine_internal.h"

using namespace mvi;

constexpr uint64_t kMaxDagRecords = 0xfffffffeull;  // the slot -> record map holds a u32, all ones: no record

// the DAG store as the kernels see it: slot | round | ibase (u64 each) | auth | kc (u32 each)
mvk::DagStore mvi::dag_view(const Dag& dg, const DevBuf& rec, const DevBuf& inc, uint64_t cap_b, uint64_t cap_i) {
  char* b = rec.as<char>();
  return mvk::DagStore{(uint64_t*)b, (uint64_t*)(b + 8 * cap_b), (uint32_t*)(b + 24 * cap_b), (uint64_t*)(b + 16 * cap_b),
                       (uint32_t*)(b + 28 * cap_b), inc.as<uint64_t>(), dg.map.as<uint32_t>(), cap_b, cap_i, dg.map_slots};
}
mvk::DagStore mvi::dag_view(const Dag& dg) { return dag_view(dg, dg.rec, dg.inc, dg.cap_b, dg.cap_i); }

// Room in the DAG store for more_b records and more_i includes on top of those there: a fresh copy,
// at least twice as large, takes the records over. Synchronises s when it grows.
mv_status mvi::dag_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, hipStream_t s, bool can_grow) {
  Dag& dg = dev.index.dag;
  const uint64_t need_b = dg.nb + more_b, need_i = dg.ni + more_i;
  if (need_b <= dg.cap_b && need_i <= dg.cap_i) return MV_OK;
  if (!can_grow)
    return set_err(ctx, MV_E_INDEX_FULL,
                   "DAG store: " + std::to_string(dg.nb) + " records + " + std::to_string(more_b) + " and " +
                       std::to_string(dg.ni) + " includes + " + std::to_string(more_i) + " that the call may add > " +
                       std::to_string(dg.cap_b) + " and " + std::to_string(dg.cap_i) + " reserved (mv_dag_reserve)");
  if (need_b > kMaxDagRecords || need_i > (1ull << 40)) return set_err(ctx, MV_E_INVALID_ARG, "too many records in the DAG store");
  const uint64_t cap_b = need_b > dg.cap_b ? std::max<uint64_t>(need_b, 2 * dg.cap_b) : dg.cap_b;
  const uint64_t cap_i = need_i > dg.cap_i ? std::max<uint64_t>(need_i, 2 * dg.cap_i) : dg.cap_i;
  DevBuf rec, inc;
  if (rec.ensure(32 * (size_t)cap_b) != hipSuccess || inc.ensure(8 * (size_t)cap_i) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "no device memory for the DAG store");
  }
  if (dg.nb) {
    const mvk::DagStore from = dag_view(dg), to = dag_view(dg, rec, inc, cap_b, cap_i);
    HIPCHK(ctx, hipMemcpyAsync(to.slot, from.slot, 8 * (size_t)dg.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.round, from.round, 8 * (size_t)dg.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.ibase, from.ibase, 8 * (size_t)dg.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.auth, from.auth, 4 * (size_t)dg.nb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(to.kc, from.kc, 4 * (size_t)dg.nb, hipMemcpyDeviceToDevice, s));
    if (dg.ni) HIPCHK(ctx, hipMemcpyAsync(to.inc, from.inc, 8 * (size_t)dg.ni, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));  // the old copy is read until here; rec and inc free it below
  std::swap(dg.rec, rec);
  std::swap(dg.inc, inc);
  dg.cap_b = cap_b, dg.cap_i = cap_i;
  return MV_OK;
}

// One seed call on stream s (include/mysti_verify.h, mv_dev_dag_seed_rows): eligibility and the counts
// that decide about room, the rows' own references towards STORED, the record rows, their includes
// towards WANTED, the include slots. Synchronises s: the eligible counts decide about room, every
// insert round reads its counter back, the record and include counts size the second half.
mv_status mvi::dag_seed_run(mv_ctx* ctx, Device& dev, const uint8_t* d_img, uint64_t size, const uint64_t* d_rows,
                            const uint8_t* d_status, uint64_t n, uint64_t floor_round, bool can_grow, hipStream_t s,
                            uint64_t* seeded) {
  Index& ix = dev.index;
  Dag& dg = ix.dag;
  memset(seeded, 0, 5 * sizeof(uint64_t));
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (n == 0) return MV_OK;
  if (n > mvk::IX_MAX_ITEMS || dg.nb + n >= kMaxDagRecords) return set_err(ctx, MV_E_INVALID_ARG, "too many rows in one seed call");
  mv_status st = order_behind_ahead(ctx, dev, s);
  if (st == MV_OK) st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_NVER, 0, 8 * (mvk::IX_CTL_STORED - mvk::IX_CTL_NVER), s));
  // per row: elig | first | kc | own_slot | rec_off
  const size_t a8 = ix_al(n), a32 = ix_al(4 * n), a64 = ix_al(8 * n);
  HIPCHK(ctx, ix.acc.ensure(2 * a8 + a32 + 2 * a64));
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(n)));
  char* b = ix.acc.as<char>();
  mvk::SeedRows r{d_img, size, d_rows, d_status, n, floor_round, (uint8_t*)b, (uint8_t*)(b + a8), (uint32_t*)(b + 2 * a8),
                  (uint64_t*)(b + 2 * a8 + a32), (uint64_t*)(b + 2 * a8 + a32 + a64)};
  HIPCHK(ctx, mvk::launch_seed_eligible(r, ix.wg.as<uint64_t>(), ctl, s));
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  const uint64_t nel = std::min<uint64_t>(h[mvk::IX_CTL_SD_ELIG], n), einc = h[mvk::IX_CTL_SD_EINC];
  const uint64_t misfit = std::min<uint64_t>(h[mvk::IX_CTL_SD_MISFIT], n);
  if (einc > mvk::IX_MAX_ITEMS) return set_err(ctx, MV_E_INVALID_ARG, "more than 2^32 includes in one seed call");
  // room for what the call may add, decided before the first insert: index and store are unchanged until here
  st = dag_room(ctx, dev, nel, einc, s, can_grow);
  if (st == MV_OK) st = index_room_for_more(ctx, dev, n + einc, can_grow, s);
  if (st != MV_OK) return st;
  if (dg.map_slots != ix.slots) return set_err(ctx, MV_E_HIP, "the DAG store's map does not match the index");
  // the rows' own references: every block of a WAL is stored (add_unloaded)
  st = insert_rounds(ctx, dev, mvk::IndexKeys{(const uint8_t*)(d_rows + 3), nullptr, 8 * mvk::SD_ROW_WORDS, 0}, n, MV_REF_STORED, s);
  if (st != MV_OK) return st;
  const uint64_t nb0 = dg.nb, ni0 = dg.ni;
  const mvk::DagStore d = dag_view(dg);
  HIPCHK(ctx, mvk::launch_seed_records(table_of(ctx, ix), ix.item.as<uint64_t>(), r, d, nb0, ni0, ix.wg.as<uint64_t>(), ctl, s));
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  const uint64_t nrec = std::min<uint64_t>(h[mvk::IX_CTL_SD_NREC], nel), ninc = std::min<uint64_t>(h[mvk::IX_CTL_SD_NINC], einc);
  uint64_t wanted = 0;
  if (nrec && ninc) {
    // the includes of the record rows: WANTED where there is no entry, and their slots
    HIPCHK(ctx, ix.keys.ensure(8 * (size_t)ninc));
    uint64_t* inc_src = ix.keys.as<uint64_t>();
    HIPCHK(ctx, mvk::launch_seed_inc_src(r, d, nb0, ni0, nrec, ninc, inc_src, ctl, s));
    st = insert_rounds(ctx, dev, mvk::IndexKeys{d_img, inc_src, 0, 1}, ninc, MV_REF_WANTED, s);
    if (st != MV_OK) return st;
    HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(ninc)));
    HIPCHK(ctx, mvk::launch_accept_missing(table_of(ctx, ix), ix.item.as<uint64_t>(), ninc, ix.wg.as<uint64_t>(), ctl, nullptr, 0, s));
    HIPCHK(ctx, mvk::launch_seed_inc(ix.item.as<uint64_t>(), d, nb0, ni0, nrec, ninc, ctl, s));
    st = read_ctl(ctx, dev, s, &h);
    if (st != MV_OK) return st;
    wanted = std::min<uint64_t>(h[mvk::IX_CTL_NMISS], ninc);
  }
  dg.nb += nrec;
  dg.ni += ninc;
  seeded[0] = n, seeded[1] = nrec, seeded[2] = ninc, seeded[3] = wanted, seeded[4] = misfit;
  return MV_OK;
}

extern "C" {

mv_status mv_dev_dag_seed_rows(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size, const uint64_t* d_blk_rows,
                               const uint8_t* d_blk_status, uint64_t n_rows, uint64_t floor_round, uint64_t* seeded,
                               void* stream) {
  if (!ctx || !seeded || (n_rows && (!d_blk_rows || !d_blk_status)) || (size && !d_wal))
    return set_err(ctx, MV_E_INVALID_ARG, "bad dag_seed_rows args");
  if ((((uintptr_t)d_wal) & 7) || (((uintptr_t)d_blk_rows) & 7))
    return set_err(ctx, MV_E_INVALID_ARG, "d_wal and d_blk_rows must be 8-byte aligned");
  memset(seeded, 0, 5 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  const mv_status st = dag_seed_run(ctx, *dev, d_wal, size, d_blk_rows, d_blk_status, n_rows, floor_round, /*can_grow=*/false, s,
                                    seeded);
  if (st != MV_OK) (void)hipStreamSynchronize(s);
  return st;
}

mv_status mv_dag_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t includes) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  Dag& dg = ix.dag;
  hipStream_t s = dev->stream;
  st = index_ctl(ctx, *dev, s);
  if (st == MV_OK) st = dag_room(ctx, *dev, blocks > dg.nb ? blocks - dg.nb : 0, includes > dg.ni ? includes - dg.ni : 0, s);
  if (st != MV_OK) return st;
  if (!dg.on && ix.slots) {  // the map of the table in force (a later table brings its own)
    HIPCHK(ctx, dg.map.ensure(4 * (size_t)ix.slots));
    dg.map_slots = ix.slots;
    HIPCHK(ctx, dg.lmark.ensure(4 * (size_t)ix.slots));  // the linearizer's marks, as long as the map
    HIPCHK(ctx, hipMemsetAsync(dg.lmark.p, 0, 4 * (size_t)ix.slots, s));
    HIPCHK(ctx, mvk::launch_dag_map(dag_view(dg), 0, ix.ctl.as<uint64_t>(), s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  dg.on = true;
  return MV_OK;
}

mv_status mv_dag_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad dag_stats args");
  memset(out, 0, 4 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  if (!ix.dag.on || !ix.ctl.p) return MV_OK;
  const uint64_t* w = nullptr;
  st = read_ctl(ctx, *dev, dev->stream, &w);
  out[0] = ix.dag.nb, out[1] = ix.dag.ni;
  if (w && ix.dag.nb && w[mvk::IX_CTL_DG_NLO]) out[2] = ~w[mvk::IX_CTL_DG_NLO], out[3] = w[mvk::IX_CTL_DG_HI];
  return st;
}

mv_status mv_dag_prune(mv_ctx* ctx, uint64_t round) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  Dag& dg = ix.dag;
  if (!dg.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  if (dg.nb == 0) return MV_OK;
  hipStream_t s = dev->stream;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  DevBuf rec, inc;
  if (rec.ensure(32 * (size_t)dg.cap_b) != hipSuccess || inc.ensure(8 * (size_t)dg.cap_i + 8) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "no device memory for the DAG store");
  }
  HIPCHK(ctx, dg.newbase.ensure(8 * (size_t)dg.nb));
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(dg.nb)));
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_DG_NI, 0, 8 * (mvk::IX_CTL_DG_NB + 1 - mvk::IX_CTL_DG_NI), s));
  HIPCHK(ctx, mvk::launch_dag_prune(dag_view(dg), dag_view(dg, rec, inc, dg.cap_b, dg.cap_i), dg.nb, round,
                                    dg.newbase.as<uint64_t>(), ix.wg.as<uint64_t>(), ctl, s));
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, *dev, s, &h);  // (synchronises: the old copy is read until here)
  if (st != MV_OK) return st;
  std::swap(dg.rec, rec);
  std::swap(dg.inc, inc);
  dg.nb = std::min<uint64_t>(h[mvk::IX_CTL_DG_NB], dg.nb);
  dg.ni = std::min<uint64_t>(h[mvk::IX_CTL_DG_NI], dg.ni);
  return MV_OK;
}

}  // extern "C"
