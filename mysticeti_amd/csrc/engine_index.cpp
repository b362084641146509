// libmysti_verify.so: the index of block references (mv_index_*) and the accept call
// (mv_accept_blocks): the host side of index.hip. The table, the insert protocol and its memory
// model are described there; where references lie in a block is block_ref.h's.
#include <string.h>

#include <algorithm>

#include "block_ref.h"
#include "engine_internal.h"

using namespace mvi;

namespace {
constexpr size_t ix_al(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr uint64_t kMinSlots = 16;
constexpr uint64_t kMaxSlots = 1ull << 38;  // an item's record holds 40 bits of slot index
constexpr size_t kSlotBytes = 64;
// rounds a call that only enqueues runs ahead (it cannot read the retry counter back): with tags
// of 32 bits or more a second round is never needed in practice; short tags (tests) need many
constexpr int kAheadRounds = 2, kAheadRoundsShortTags = 64;
constexpr int kMaxRounds = 1 << 16;

using Index = Device::Index;
using Pending = Device::Index::Pending;
using Dag = Device::Index::Dag;
constexpr uint64_t kMaxDagRecords = 0xfffffffeull;  // the slot -> record map holds a u32, all ones: no record
constexpr uint64_t kMaxDecideWaves = 1ull << 26;

// the DAG store as the kernels see it: slot | round | ibase (u64 each) | auth | kc (u32 each)
mvk::DagStore dag_view(const Dag& dg, const DevBuf& rec, const DevBuf& inc, uint64_t cap_b, uint64_t cap_i) {
  char* b = rec.as<char>();
  return mvk::DagStore{(uint64_t*)b, (uint64_t*)(b + 8 * cap_b), (uint32_t*)(b + 24 * cap_b), (uint64_t*)(b + 16 * cap_b),
                       (uint32_t*)(b + 28 * cap_b), inc.as<uint64_t>(), dg.map.as<uint32_t>(), cap_b, cap_i, dg.map_slots};
}
mvk::DagStore dag_view(const Dag& dg) { return dag_view(dg, dg.rec, dg.inc, dg.cap_b, dg.cap_i); }

// copy k of the suspended-block store as the kernels see it
mvk::PendStore pend_view(const Pending& pd, int k) {
  char* b = pd.blk[k].as<char>();
  return mvk::PendStore{(uint64_t*)b, (uint64_t*)(b + 8 * pd.cap_b), (uint64_t*)(b + 16 * pd.cap_b),
                        (uint32_t*)(b + 24 * pd.cap_b), pd.inc[k].as<uint64_t>()};
}

// slots (a power of two) so that `entries` entries load the table to 1/2 at most; 0: too many
uint64_t slots_for(uint64_t entries) {
  if (entries > kMaxSlots / 2) return 0;
  uint64_t s = kMinSlots;
  while (s / 2 < entries) s <<= 1;
  return s;
}

mvk::IndexTable table_of(mv_ctx* ctx, const Index& ix) {
  return mvk::IndexTable{ix.slots ? ix.tab.as<unsigned long long>() : nullptr, ix.slots ? ix.slots - 1 : 0,
                         ctx->index_secret[0], ctx->index_secret[1], ix.tag_bits};
}

uint32_t wanted_tag_bits(mv_ctx* ctx) { return (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, ctx->kn.index_tag_bits)); }

// the control words and their pinned mirror, made (and zeroed) on first use
mv_status index_ctl(mv_ctx* ctx, Device& dev, hipStream_t s) {
  Index& ix = dev.index;
  if (ix.ctl.p) return MV_OK;
  HIPCHK(ctx, ix.ctl.ensure(8 * mvk::IX_CTL_WORDS));
  HIPCHK(ctx, ix.h_ctl.ensure(8 * mvk::IX_CTL_WORDS));
  HIPCHK(ctx, hipMemsetAsync(ix.ctl.p, 0, 8 * mvk::IX_CTL_WORDS, s));
  return MV_OK;
}

// The control words on the host (synchronises s). The entry count becomes exact; a probe that ran
// through the table, or items a call gave up on, is an error.
mv_status read_ctl(mv_ctx* ctx, Device& dev, hipStream_t s, const uint64_t** words) {
  Index& ix = dev.index;
  HIPCHK(ctx, hipMemcpyAsync(ix.h_ctl.p, ix.ctl.p, 8 * mvk::IX_CTL_WORDS, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  const uint64_t* w = ix.h_ctl.as<uint64_t>();
  if (words) *words = w;
  ix.used = w[mvk::IX_CTL_HAVE] + w[mvk::IX_CTL_WANTED];
  ix.used_exact = true;
  if (w[mvk::IX_CTL_ERR])
    return set_err(ctx, MV_E_HIP,
                   "index: " + std::to_string(w[mvk::IX_CTL_ERR]) +
                       " probes gave up (the table was full, or an insert that was enqueued ahead met more tag "
                       "collisions than its rounds); mv_index_clear resets it");
  return MV_OK;
}

// A table of `slots` slots with the tag width now asked for; the entries of the one in force are
// rehashed into it on the device. Synchronises s.
mv_status index_resize(mv_ctx* ctx, Device& dev, uint64_t slots, hipStream_t s) {
  Index& ix = dev.index;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  DevBuf fresh;
  if (fresh.ensure(kSlotBytes * slots) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(ctx, MV_E_ALLOC, "index: no device memory for " + std::to_string(slots) + " slots");
  }
  HIPCHK(ctx, hipMemsetAsync(fresh.p, 0, kSlotBytes * slots, s));
  const uint64_t old_slots = ix.slots;
  const uint32_t bits = wanted_tag_bits(ctx);
  if (old_slots) {
    const mvk::IndexTable nt{fresh.as<unsigned long long>(), slots - 1, ctx->index_secret[0], ctx->index_secret[1], bits};
    HIPCHK(ctx, mvk::launch_index_rebuild(ix.tab.as<uint64_t>(), old_slots, nt, ix.ctl.as<uint64_t>(), s));
    // the suspended-block store holds slots of the old table
    const Pending& pd = ix.pend;
    if (pd.nb) {
      const mvk::PendStore p = pend_view(pd, pd.cur);
      HIPCHK(ctx, mvk::launch_pend_reresolve(ix.tab.as<uint64_t>(), nt, p.slot, pd.nb, ix.ctl.as<uint64_t>(), s));
      HIPCHK(ctx, mvk::launch_pend_reresolve(ix.tab.as<uint64_t>(), nt, p.inc, pd.ni, ix.ctl.as<uint64_t>(), s));
    }
    // ... and so does the DAG store
    const Dag& dg = ix.dag;
    if (dg.on && dg.nb) {
      const mvk::DagStore d = dag_view(dg);
      HIPCHK(ctx, mvk::launch_pend_reresolve(ix.tab.as<uint64_t>(), nt, d.slot, dg.nb, ix.ctl.as<uint64_t>(), s));
      HIPCHK(ctx, mvk::launch_pend_reresolve(ix.tab.as<uint64_t>(), nt, d.inc, dg.ni, ix.ctl.as<uint64_t>(), s));
    }
  }
  // its slot -> record map is as long as the table: a fresh one, filled from the re-resolved slots
  DevBuf fresh_map;
  if (ix.dag.on) {
    if (fresh_map.ensure(4 * (size_t)slots) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      return set_err(ctx, MV_E_ALLOC, "no device memory for the DAG store's map");
    }
    mvk::DagStore d = dag_view(ix.dag);
    d.map = fresh_map.as<uint32_t>(), d.n_slots = slots;
    HIPCHK(ctx, mvk::launch_dag_map(d, ix.dag.nb, ix.ctl.as<uint64_t>(), s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));  // the old table is read until here; `fresh` frees it below
  if (ix.dag.on) {
    std::swap(ix.dag.map, fresh_map);
    ix.dag.map_slots = slots;
  }
  std::swap(ix.tab, fresh);
  ix.slots = slots;
  ix.tag_bits = bits;
  if (old_slots) ix.rebuilds++;
  return MV_OK;
}

// Orders stream s behind the last insert that was only enqueued (device-side wait)
mv_status order_behind_ahead(mv_ctx* ctx, Device& dev, hipStream_t s) {
  if (dev.index.ahead_set) HIPCHK(ctx, hipStreamWaitEvent(s, dev.index.ahead, 0));
  return MV_OK;
}

// Room for `more` entries on top of those there; the count is made exact before the table grows.
mv_status index_room_for_more(mv_ctx* ctx, Device& dev, uint64_t more, bool can_grow, hipStream_t s) {
  Index& ix = dev.index;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  if (ix.used + more > ix.slots / 2 && !ix.used_exact) {
    st = read_ctl(ctx, dev, s, nullptr);
    if (st != MV_OK) return st;
  }
  if (ix.used + more <= ix.slots / 2) return MV_OK;
  if (!can_grow)
    return set_err(ctx, MV_E_INDEX_FULL,
                   "index: " + std::to_string(ix.used) + " entries + " + std::to_string(more) + " that the call may add > " +
                       std::to_string(ix.slots / 2) + " reserved (mv_index_reserve)");
  const uint64_t need = slots_for(std::max(ix.used + more, ix.slots));  // at least twice the slots
  if (!need) return set_err(ctx, MV_E_INVALID_ARG, "index: too many entries");
  return index_resize(ctx, dev, need, s);
}

// Insert rounds of n items towards `state` with the counter read back after each (synchronises s)
mv_status insert_rounds(mv_ctx* ctx, Device& dev, const mvk::IndexKeys& ks, uint64_t n, uint32_t state, hipStream_t s) {
  Index& ix = dev.index;
  if (n == 0) return MV_OK;
  HIPCHK(ctx, ix.item.ensure(8 * (size_t)n, ix.ahead));
  const mvk::IndexTable t = table_of(ctx, ix);
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  for (int round = 0;; round++) {
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_RETRY, 0, 8, s));
    HIPCHK(ctx, mvk::launch_index_round(t, ks, n, ix.item.as<uint64_t>(), state, round, ctl, s));
    const uint64_t* w = nullptr;
    const mv_status st = read_ctl(ctx, dev, s, &w);
    if (st != MV_OK) return st;
    if (w[mvk::IX_CTL_RETRY] == 0) return MV_OK;
    if (round >= kMaxRounds) return set_err(ctx, MV_E_HIP, "index: an insert did not settle (tag collisions)");
  }
}

bool state_ok(uint32_t state) { return state == MV_REF_WANTED || state == MV_REF_HAVE; }

// Room in the suspended-block store for more_b blocks and more_i includes on top of those there.
// Growing keeps the records of the copy in force. Synchronises s when it grows.
mv_status pending_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, bool can_grow, hipStream_t s) {
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

// Room in the DAG store for more_b records and more_i includes on top of those there: a fresh copy,
// at least twice as large, takes the records over. Synchronises s when it grows.
mv_status dag_room(mv_ctx* ctx, Device& dev, uint64_t more_b, uint64_t more_i, hipStream_t s, bool can_grow = true) {
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

// Where accept_run leaves its results (device memory of dev.index)
struct AcceptOut {
  uint64_t n_missing = 0;
  const uint8_t *status = nullptr, *state = nullptr;
  const uint64_t* missing = nullptr;
  // for the connect call: the call's arrays, the candidates (their slots are in pend.cand_slot) and
  // their includes (whose insert's records are in index.item)
  mvk::AcceptArrays a{};
  uint64_t ncand = 0, ninc = 0;
};

// One accept call on stream s (include/mysti_verify.h, mv_accept_blocks). Synchronises s: the
// count of blocks to verify sizes the pipeline's launches, the candidate and include counts size
// the lists and decide about room, every insert round reads its counter back, and the missing
// total ends the call.
mv_status accept_run(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                     const uint64_t* d_len, const uint64_t* d_grp, uint32_t n32, uint64_t cap_missing, bool can_grow,
                     hipStream_t s, AcceptOut& out, bool connect = false) {
  Index& ix = dev.index;
  out = AcceptOut();
  const size_t n = n32;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_NVER, 0, 8 * (mvk::IX_CTL_STORED - mvk::IX_CTL_NVER), s));
  // per block: known | status | state | rank | gidx | gflag | kc | cand_blk | cand_src | inc_base
  const size_t a8 = ix_al(n), a32 = ix_al(4 * n), a64 = ix_al(8 * n), nwg = mvk::index_groups(n), w64 = ix_al(8 * nwg);
  HIPCHK(ctx, ix.acc.ensure(3 * a8 + 5 * a32 + 2 * a64));
  HIPCHK(ctx, ix.accv.ensure(2 * a64 + a8));
  HIPCHK(ctx, ix.wg.ensure(4 * w64));
  char* b = ix.acc.as<char>();
  char* v = ix.accv.as<char>();
  char* w = ix.wg.as<char>();
  mvk::AcceptArrays a{};
  a.buf = d_buf, a.buf_bytes = buf_bytes, a.off = d_off, a.len = d_len, a.grp = d_grp, a.n = n;
  a.known = (uint8_t*)b, a.status = (uint8_t*)(b + a8), a.state = (uint8_t*)(b + 2 * a8);
  char* b32 = b + 3 * a8;
  a.rank = (uint32_t*)b32, a.gidx = (uint32_t*)(b32 + a32), a.gflag = (uint32_t*)(b32 + 2 * a32);
  a.kc = (uint32_t*)(b32 + 3 * a32), a.cand_blk = (uint32_t*)(b32 + 4 * a32);
  a.cand_src = (uint64_t*)(b32 + 5 * a32), a.inc_base = (uint64_t*)(b32 + 5 * a32 + a64);
  a.v_off = (uint64_t*)v, a.v_len = (uint64_t*)(v + a64), a.v_status = (uint8_t*)(v + 2 * a64);
  a.wg_a = (uint64_t*)w, a.wg_b = (uint64_t*)(w + w64), a.base_a = (uint64_t*)(w + 2 * w64), a.base_b = (uint64_t*)(w + 3 * w64);
  HIPCHK(ctx, hipMemsetAsync(a.gflag, 0, 4 * n, s));
  // 1. probe: KNOWN blocks, the list of the others
  HIPCHK(ctx, mvk::launch_accept_probe(table_of(ctx, ix), a, ctl, s));
  const uint64_t* h = nullptr;
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  const uint64_t nver = std::min<uint64_t>(h[mvk::IX_CTL_NVER], n);
  // 2. verify: the block path as mv_dev_verify_blocks runs it, in chunks of at most max_batch blocks
  for (uint64_t i = 0; i < nver;) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(nver - i, ctx->max_batch);
    st = enqueue_blocks(ctx, dev, d_buf, buf_bytes, a.v_off + i, a.v_len + i, m, a.v_status + i, nullptr, nullptr, s);
    if (st != MV_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
    i += m;
  }
  // 3. groups, states, the candidates and their include counts
  HIPCHK(ctx, mvk::launch_accept_groups(a, ctl, s));
  st = read_ctl(ctx, dev, s, &h);
  poll_flags(ctx, dev);
  if (st != MV_OK) return st;
  const uint64_t ncand = std::min<uint64_t>(h[mvk::IX_CTL_NCAND], n), ninc = h[mvk::IX_CTL_NINC];
  if (ninc > mvk::IX_MAX_ITEMS) return set_err(ctx, MV_E_INVALID_ARG, "more than 2^32 includes in one accept call");
  out.status = a.status;
  out.state = a.state;
  out.a = a;
  if (ncand == 0) return MV_OK;
  // room for what the call may add, decided before the first insert (the index is unchanged until
  // here; a connect call that cannot grow asks the store first, which leaves both as they are)
  if (connect) {
    st = pending_room(ctx, dev, ncand, ninc, can_grow, s);
    if (st != MV_OK) return st;
  }
  st = index_room_for_more(ctx, dev, ncand + ninc, can_grow, s);
  if (st != MV_OK) return st;
  out.ncand = ncand;
  // 4. own references of the candidates: NEW / DUP, HAVE
  st = insert_rounds(ctx, dev, mvk::IndexKeys{d_buf, a.cand_src, 0, 1}, ncand, MV_REF_HAVE, s);
  if (st != MV_OK) return st;
  HIPCHK(ctx, mvk::launch_accept_own_states(a, ix.item.as<uint64_t>(), ncand, s));
  if (connect) {
    HIPCHK(ctx, ix.pend.cand_slot.ensure(8 * (size_t)ncand));
    HIPCHK(ctx, mvk::launch_pend_own_slots(ix.item.as<uint64_t>(), ncand, ix.pend.cand_slot.as<uint64_t>(), s));
  }
  if (ninc == 0) return MV_OK;
  out.ninc = ninc;
  // 5. includes of the NEW blocks: WANTED, the missing list
  HIPCHK(ctx, ix.keys.ensure(8 * (size_t)ninc));
  uint64_t* inc_src = ix.keys.as<uint64_t>();
  HIPCHK(ctx, mvk::launch_accept_inc_src(a, ncand, ninc, inc_src, s));
  st = insert_rounds(ctx, dev, mvk::IndexKeys{d_buf, inc_src, 0, 1}, ninc, MV_REF_WANTED, s);
  if (st != MV_OK) return st;
  const uint64_t capd = std::min(cap_missing, ninc);
  const size_t iwg = mvk::index_groups(ninc), i64 = ix_al(8 * iwg);
  HIPCHK(ctx, ix.wg.ensure(2 * i64));
  HIPCHK(ctx, ix.miss.ensure(48 * (size_t)capd + 8));
  HIPCHK(ctx, mvk::launch_accept_missing(table_of(ctx, ix), ix.item.as<uint64_t>(), ninc, ix.wg.as<uint64_t>(),
                                         (uint64_t*)(ix.wg.as<char>() + i64), ctl, ix.miss.as<uint64_t>(), capd, s));
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  out.n_missing = h[mvk::IX_CTL_NMISS];
  out.missing = ix.miss.as<uint64_t>();
  return MV_OK;
}

// the first device of the context, ready for an index call on its own stream
mv_status index_dev(mv_ctx* ctx, Device*& dev) {
  dev = &ctx->devs[0];
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  return order_behind_ahead(ctx, *dev, dev->stream);
}

// The host-buffer calls' way in: the blocks' bytes and the off | len | grp table go to the device,
// then accept_run.
mv_status stage_blocks(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                       const uint64_t* grp, uint32_t n, uint64_t cap_missing, hipStream_t s, AcceptOut& ao, bool connect) {
  Index& ix = dev.index;
  // the bytes: pinned, in order and disjoint blocks as one DMA of the caller's memory in place;
  // else packed block by block (8-byte aligned, which also separates overlapping blocks)
  uint64_t bytes = 0, span = 0;
  const uint64_t first = off[0];
  bool direct = host_pinned(buf + first);
  for (uint32_t k = 0; k < n; k++) {
    bytes += (len[k] + 7) & ~7ull;
    if (direct && (off[k] < first || off[k] - first < span)) direct = false;
    if (direct) span = off[k] - first + len[k];
  }
  direct = direct && span && span <= 2 * bytes + 4096 && pinned_range_holds(buf + first, span);
  const uint64_t buf_bytes = direct ? span : bytes;
  const size_t nn = n;
  std::vector<uint64_t> tab((grp ? 3 : 2) * nn);  // device offsets | lengths | groups
  HIPCHK(ctx, ix.in.ensure(buf_bytes + 32));
  uint8_t* d_buf = ix.in.as<uint8_t>();
  if (direct) {
    for (size_t k = 0; k < nn; k++) tab[k] = off[k] - first;
    HIPCHK(ctx, hipMemcpyAsync(d_buf, buf + first, span, hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(ctx, dev.hc.h_in.ensure(bytes + 32));
    uint8_t* h = dev.hc.h_in.as<uint8_t>();
    uint64_t p = 0;
    for (size_t k = 0; k < nn; k++) {
      const uint64_t l = len[k], pl = (l + 7) & ~7ull;
      if (l) memcpy(h + p, buf + off[k], l);
      memset(h + p + l, 0, pl - l);
      tab[k] = p;
      p += pl;
    }
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(d_buf, h, bytes, hipMemcpyHostToDevice, s));
  }
  HIPCHK(ctx, hipMemsetAsync(d_buf + buf_bytes, 0, 32, s));  // the readable bytes past the last block
  memcpy(tab.data() + nn, len, 8 * nn);
  if (grp) memcpy(tab.data() + 2 * nn, grp, 8 * nn);
  HIPCHK(ctx, ix.tab_in.ensure(8 * tab.size()));
  HIPCHK(ctx, hipMemcpyAsync(ix.tab_in.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, s));
  const uint64_t* d_tab = ix.tab_in.as<uint64_t>();
  return accept_run(ctx, dev, d_buf, buf_bytes, d_tab, d_tab + nn, grp ? d_tab + 2 * nn : nullptr, n, cap_missing,
                  /*can_grow=*/true, s, ao, connect);
}

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
    const size_t w64 = 8 * mvk::index_groups(ao.ncand);
    HIPCHK(ctx, ix.wg.ensure(4 * w64));
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
  HIPCHK(ctx, ix.wg.ensure(4 * 8 * mvk::index_groups(nb)));
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

// One decide call on stream s (include/mysti_verify.h, mv_decide_leaders): the rows sorted by round
// on the host, k_dg_pick, the counts of voting and decision records read back (they size the
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
  HIPCHK(ctx, ix.wg.ensure(4 * 8 * mvk::index_groups(nb) + 8));
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

// mv_index_insert / mv_index_insert_stored
mv_status index_insert_host(mv_ctx* ctx, const uint64_t* refs, uint64_t n, uint32_t state, uint8_t* prior) {
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  hipStream_t s = dev->stream;
  st = index_room_for_more(ctx, *dev, n, /*can_grow=*/true, s);
  if (st != MV_OK) return st;
  HIPCHK(ctx, ix.keys.ensure(48 * (size_t)n));
  HIPCHK(ctx, hipMemcpyAsync(ix.keys.p, refs, 48 * (size_t)n, hipMemcpyHostToDevice, s));
  st = insert_rounds(ctx, *dev, mvk::IndexKeys{ix.keys.as<uint8_t>(), nullptr, 48, 0}, n, state, s);
  if (st != MV_OK) return st;
  if (prior) {
    HIPCHK(ctx, ix.out.ensure((size_t)n));
    HIPCHK(ctx, mvk::launch_index_prior(ix.item.as<uint64_t>(), n, ix.out.as<uint8_t>(), s));
    HIPCHK(ctx, hipMemcpyAsync(prior, ix.out.p, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return MV_OK;
}
}  // namespace

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
  const size_t a8 = ix_al(n), a32 = ix_al(4 * n), a64 = ix_al(8 * n), w64 = 8 * mvk::index_groups(n);
  HIPCHK(ctx, ix.acc.ensure(2 * a8 + a32 + 2 * a64));
  HIPCHK(ctx, ix.wg.ensure(4 * w64));
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
    const size_t i64 = ix_al(8 * mvk::index_groups(ninc));
    HIPCHK(ctx, ix.wg.ensure(2 * i64));
    HIPCHK(ctx, mvk::launch_accept_missing(table_of(ctx, ix), ix.item.as<uint64_t>(), ninc, ix.wg.as<uint64_t>(),
                                           (uint64_t*)(ix.wg.as<char>() + i64), ctl, nullptr, 0, s));
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

mv_status mv_index_reserve(mv_ctx* ctx, uint64_t entries) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  const uint64_t need = slots_for(entries);
  if (!need) return set_err(ctx, MV_E_INVALID_ARG, "index: too many entries");
  if (ix.slots >= need && ix.tag_bits == wanted_tag_bits(ctx)) return MV_OK;
  return index_resize(ctx, *dev, std::max(need, ix.slots), dev->stream);
}

mv_status mv_index_clear(mv_ctx* ctx) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  ix.pend.nb = ix.pend.ni = ix.pend.levels = 0;  // the store's records are slots of the table
  ix.dag.nb = ix.dag.ni = 0;                     // ... and so are the DAG store's
  if (!ix.slots) return MV_OK;
  if (ix.dag.on && ix.dag.map_slots)
    HIPCHK(ctx, hipMemsetAsync(ix.dag.map.p, 0xff, 4 * (size_t)ix.dag.map_slots, dev->stream));
  HIPCHK(ctx, hipMemsetAsync(ix.tab.p, 0, kSlotBytes * ix.slots, dev->stream));
  HIPCHK(ctx, hipMemsetAsync(ix.ctl.p, 0, 8 * mvk::IX_CTL_WORDS, dev->stream));
  HIPCHK(ctx, hipStreamSynchronize(dev->stream));
  ix.used = 0;
  ix.used_exact = true;
  ix.tag_bits = wanted_tag_bits(ctx);
  return MV_OK;
}

mv_status mv_index_stats(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad index_stats args");
  memset(out, 0, 5 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  if (!ix.ctl.p) return MV_OK;
  const uint64_t* w = nullptr;
  st = read_ctl(ctx, *dev, dev->stream, &w);
  out[0] = w ? w[mvk::IX_CTL_HAVE] : 0;
  out[1] = w ? w[mvk::IX_CTL_WANTED] : 0;
  out[2] = ix.slots / 2;
  out[3] = ix.rebuilds;
  out[4] = w ? w[mvk::IX_CTL_MAXPROBE] : 0;
  return st;
}

mv_status mv_index_insert(mv_ctx* ctx, const uint64_t* refs, uint64_t n, uint32_t state, uint8_t* prior) {
  if (!ctx || (n && !refs) || !state_ok(state) || n > mvk::IX_MAX_ITEMS)
    return set_err(ctx, MV_E_INVALID_ARG, "bad index_insert args");
  return index_insert_host(ctx, refs, n, state, prior);
}

mv_status mv_index_insert_stored(mv_ctx* ctx, const uint64_t* refs, uint64_t n, uint8_t* prior) {
  if (!ctx || (n && !refs) || n > mvk::IX_MAX_ITEMS) return set_err(ctx, MV_E_INVALID_ARG, "bad index_insert_stored args");
  return index_insert_host(ctx, refs, n, MV_REF_STORED, prior);
}

mv_status mv_index_lookup(mv_ctx* ctx, const uint64_t* refs, uint64_t n, uint8_t* state) {
  if (!ctx || (n && (!refs || !state))) return set_err(ctx, MV_E_INVALID_ARG, "bad index_lookup args");
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  if (!ix.slots) {
    memset(state, MV_REF_ABSENT, (size_t)n);
    return MV_OK;
  }
  hipStream_t s = dev->stream;
  HIPCHK(ctx, ix.keys.ensure(48 * (size_t)n));
  HIPCHK(ctx, ix.out.ensure((size_t)n));
  HIPCHK(ctx, hipMemcpyAsync(ix.keys.p, refs, 48 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, mvk::launch_index_lookup(table_of(ctx, ix), mvk::IndexKeys{ix.keys.as<uint8_t>(), nullptr, 48, 0}, n,
                                       ix.out.as<uint8_t>(), ix.ctl.as<uint64_t>(), s));
  HIPCHK(ctx, hipMemcpyAsync(state, ix.out.p, (size_t)n, hipMemcpyDeviceToHost, s));
  return read_ctl(ctx, *dev, s, nullptr);
}

mv_status mv_index_wanted(mv_ctx* ctx, uint64_t* refs, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !refs)) return set_err(ctx, MV_E_INVALID_ARG, "bad index_wanted args");
  *n = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  Index& ix = dev->index;
  if (!ix.slots) return MV_OK;
  hipStream_t s = dev->stream;
  const uint64_t capd = std::min(cap, ix.slots);
  const size_t nwg = mvk::index_groups(ix.slots), w64 = ix_al(8 * nwg);
  HIPCHK(ctx, ix.wg.ensure(2 * w64));
  HIPCHK(ctx, ix.miss.ensure(48 * (size_t)capd + 8));
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  HIPCHK(ctx, mvk::launch_index_wanted(table_of(ctx, ix), ix.wg.as<uint64_t>(), (uint64_t*)(ix.wg.as<char>() + w64),
                                       ctl + mvk::IX_CTL_NWANTED, ix.miss.as<uint64_t>(), capd, s));
  const uint64_t* w = nullptr;
  st = read_ctl(ctx, *dev, s, &w);
  if (st != MV_OK) return st;
  const uint64_t total = w[mvk::IX_CTL_NWANTED], wr = std::min(total, capd);
  if (wr) {
    HIPCHK(ctx, hipMemcpyAsync(refs, ix.miss.p, 48 * (size_t)wr, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  *n = total;
  return MV_OK;
}

mv_status mv_accept_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, const uint64_t* grp,
                           uint32_t n, uint8_t* blk_status, uint8_t* blk_state, uint64_t* missing, uint64_t cap_missing,
                           uint64_t* n_missing) {
  if (!ctx || !n_missing || (n && (!buf || !off || !len || !blk_status || !blk_state)) || (cap_missing && !missing))
    return set_err(ctx, MV_E_INVALID_ARG, "bad accept args");
  *n_missing = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  if (n == 0) return MV_OK;
  Device* dev;
  mv_status st = index_dev(ctx, dev);
  if (st != MV_OK) return st;
  hipStream_t s = dev->stream;
  const size_t nn = n;
  AcceptOut ao;
  st = stage_blocks(ctx, *dev, buf, off, len, grp, n, cap_missing, s, ao, /*connect=*/false);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);  // (the copies above may still be in flight)
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(blk_status, ao.status, nn, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(blk_state, ao.state, nn, hipMemcpyDeviceToHost, s));
  const uint64_t wr = std::min(ao.n_missing, cap_missing);
  if (wr) HIPCHK(ctx, hipMemcpyAsync(missing, ao.missing, 48 * (size_t)wr, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *n_missing = ao.n_missing;
  return MV_OK;
}

mv_status mv_dev_accept_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                               const uint64_t* d_len, const uint64_t* d_grp, uint32_t n, uint8_t* d_blk_status,
                               uint8_t* d_blk_state, uint64_t* d_missing, uint64_t cap_missing, uint64_t* n_missing,
                               void* stream) {
  if (!ctx || !n_missing || (n && (!d_buf || !d_off || !d_len || !d_blk_status || !d_blk_state)) ||
      (cap_missing && !d_missing))
    return set_err(ctx, MV_E_INVALID_ARG, "bad accept args");
  if (((uintptr_t)d_buf) & 7) return set_err(ctx, MV_E_INVALID_ARG, "d_buf must be 8-byte aligned");
  *n_missing = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st != MV_OK) return st;
  AcceptOut ao;
  st = accept_run(ctx, *dev, d_buf, buf_bytes, d_off, d_len, d_grp, n, cap_missing, /*can_grow=*/false, s, ao);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(ctx, hipMemcpyAsync(d_blk_status, ao.status, (size_t)n, hipMemcpyDeviceToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(d_blk_state, ao.state, (size_t)n, hipMemcpyDeviceToDevice, s));
  const uint64_t wr = std::min(ao.n_missing, cap_missing);
  if (wr) HIPCHK(ctx, hipMemcpyAsync(d_missing, ao.missing, 48 * (size_t)wr, hipMemcpyDeviceToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *n_missing = ao.n_missing;
  return MV_OK;
}

mv_status mv_dev_index_insert(mv_ctx* ctx, int device, const uint64_t* d_words, uint64_t stride_words, uint64_t n,
                              uint32_t state, void* stream) {
  if (!ctx || (n && !d_words) || stride_words < mv::br::KEY_WORDS || !(state_ok(state) || state == MV_REF_STORED) ||
      n > mvk::IX_MAX_ITEMS ||
      (((uintptr_t)d_words) & 7))
    return set_err(ctx, MV_E_INVALID_ARG, "bad index_insert args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "the index lives on the context's first device");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  Index& ix = dev->index;
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  mv_status st = order_behind_ahead(ctx, *dev, s);
  if (st == MV_OK) st = index_room_for_more(ctx, *dev, n, /*can_grow=*/false, s);
  if (st != MV_OK) return st;
  // the per-item records: every other index call is synchronous and has finished; the last
  // enqueued insert is ahead of this one on s (the wait above) and guards the buffer if it grows
  HIPCHK(ctx, ix.item.ensure(8 * (size_t)n, ix.ahead));
  const mvk::IndexTable t = table_of(ctx, ix);
  const mvk::IndexKeys ks{(const uint8_t*)d_words, nullptr, 8 * stride_words, 0};
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  const int rounds = ix.tag_bits >= 32 ? kAheadRounds : kAheadRoundsShortTags;
  for (int round = 0; round < rounds; round++) {
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_RETRY, 0, 8, s));
    HIPCHK(ctx, mvk::launch_index_round(t, ks, n, ix.item.as<uint64_t>(), state, round, ctl, s));
  }
  HIPCHK(ctx, mvk::launch_index_giveup(ctl, s));
  HIPCHK(ctx, ix.ahead.ensure());
  HIPCHK(ctx, hipEventRecord(ix.ahead, s));
  ix.ahead_set = true;
  ix.used += n;
  ix.used_exact = false;
  return MV_OK;
}


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
  HIPCHK(ctx, ix.wg.ensure(4 * 8 * mvk::index_groups(dg.nb)));
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
