// libmysti_verify.so: the index of block references (mv_index_*) and the accept call
// (mv_accept_blocks): the host side of index.hip. The table, the insert protocol and its memory
// model are described in index_dev.h; where references lie in a block is block_ref.h's.
#include <string.h>

#include <algorithm>

#include "block_ref.h"
#include "engine_internal.h"

using namespace mvi;

namespace {
constexpr uint64_t kMinSlots = 16;
constexpr uint64_t kMaxSlots = 1ull << 38;  // an item's record holds 40 bits of slot index
constexpr size_t kSlotBytes = 64;
// rounds a call that only enqueues runs ahead (it cannot read the retry counter back): with tags
// of 32 bits or more a second round is never needed in practice; short tags (tests) need many
constexpr int kAheadRounds = 2, kAheadRoundsShortTags = 64;
constexpr int kMaxRounds = 1 << 16;


// slots (a power of two) so that `entries` entries load the table to 1/2 at most; 0: too many
uint64_t slots_for(uint64_t entries) {
  if (entries > kMaxSlots / 2) return 0;
  uint64_t s = kMinSlots;
  while (s / 2 < entries) s <<= 1;
  return s;
}

uint32_t wanted_tag_bits(mv_ctx* ctx) { return (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, ctx->kn.index_tag_bits)); }

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
      HIPCHK(ctx, mvk::launch_index_reresolve(ix.tab.as<uint64_t>(), old_slots, nt, p.slot, pd.nb, ix.ctl.as<uint64_t>(), s));
      HIPCHK(ctx, mvk::launch_index_reresolve(ix.tab.as<uint64_t>(), old_slots, nt, p.inc, pd.ni, ix.ctl.as<uint64_t>(), s));
    }
    // ... and so does the DAG store
    const Dag& dg = ix.dag;
    if (dg.on && dg.nb) {
      const mvk::DagStore d = dag_view(dg);
      HIPCHK(ctx, mvk::launch_index_reresolve(ix.tab.as<uint64_t>(), old_slots, nt, d.slot, dg.nb, ix.ctl.as<uint64_t>(), s));
      HIPCHK(ctx, mvk::launch_index_reresolve(ix.tab.as<uint64_t>(), old_slots, nt, d.inc, dg.ni, ix.ctl.as<uint64_t>(), s));
    }
    // ... and the proposer's state
    if (ix.prop.on) {
      st = propose_follow_table(ctx, dev, old_slots, nt, s);
      if (st != MV_OK) {
        (void)hipStreamSynchronize(s);
        return st;
      }
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
  // ... and so are the linearizer's committed marks, which follow their keys into the new table
  DevBuf fresh_mark;
  if (ix.dag.on) {
    const mvk::IndexTable nt{fresh.as<unsigned long long>(), slots - 1, ctx->index_secret[0], ctx->index_secret[1], bits};
    st = linear_marks_for(ctx, dev, old_slots, nt, slots, fresh_mark, s);
    if (st != MV_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(s));  // the old table is read until here; `fresh` frees it below
  if (ix.dag.on) {
    std::swap(ix.dag.map, fresh_map);
    std::swap(ix.dag.lmark, fresh_mark);
    ix.dag.map_slots = slots;
  }
  std::swap(ix.tab, fresh);
  ix.slots = slots;
  ix.tag_bits = bits;
  if (old_slots) ix.rebuilds++;
  return MV_OK;
}

bool state_ok(uint32_t state) { return state == MV_REF_WANTED || state == MV_REF_HAVE; }

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

mvk::IndexTable mvi::table_of(mv_ctx* ctx, const Index& ix) {
  return mvk::IndexTable{ix.slots ? ix.tab.as<unsigned long long>() : nullptr, ix.slots ? ix.slots - 1 : 0,
                         ctx->index_secret[0], ctx->index_secret[1], ix.tag_bits};
}

// the control words and their pinned mirror, made (and zeroed) on first use
mv_status mvi::index_ctl(mv_ctx* ctx, Device& dev, hipStream_t s) {
  Index& ix = dev.index;
  if (ix.ctl.p) return MV_OK;
  HIPCHK(ctx, ix.ctl.ensure(8 * mvk::IX_CTL_WORDS));
  HIPCHK(ctx, ix.h_ctl.ensure(8 * mvk::IX_CTL_WORDS));
  HIPCHK(ctx, hipMemsetAsync(ix.ctl.p, 0, 8 * mvk::IX_CTL_WORDS, s));
  return MV_OK;
}

// The control words on the host (synchronises s). The entry count becomes exact; a probe that ran
// through the table, or items a call gave up on, is an error.
mv_status mvi::read_ctl(mv_ctx* ctx, Device& dev, hipStream_t s, const uint64_t** words) {
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

// Orders stream s behind the last insert that was only enqueued (device-side wait)
mv_status mvi::order_behind_ahead(mv_ctx* ctx, Device& dev, hipStream_t s) {
  if (dev.index.ahead_set) HIPCHK(ctx, hipStreamWaitEvent(s, dev.index.ahead, 0));
  return MV_OK;
}

// Room for `more` entries on top of those there; the count is made exact before the table grows.
mv_status mvi::index_room_for_more(mv_ctx* ctx, Device& dev, uint64_t more, bool can_grow, hipStream_t s) {
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
mv_status mvi::insert_rounds(mv_ctx* ctx, Device& dev, const mvk::IndexKeys& ks, uint64_t n, uint32_t state, hipStream_t s) {
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

// One accept call on stream s (include/mysti_verify.h, mv_accept_blocks). Synchronises s: the
// count of blocks to verify sizes the pipeline's launches, the candidate and include counts size
// the lists and decide about room, every insert round reads its counter back, and the missing
// total ends the call.
mv_status mvi::accept_run(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                     const uint64_t* d_len, const uint64_t* d_grp, uint32_t n32, uint64_t cap_missing, bool can_grow,
                          hipStream_t s, AcceptOut& out, bool connect) {
  Index& ix = dev.index;
  out = AcceptOut();
  const size_t n = n32;
  mv_status st = index_ctl(ctx, dev, s);
  if (st != MV_OK) return st;
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::IX_CTL_NVER, 0, 8 * (mvk::IX_CTL_STORED - mvk::IX_CTL_NVER), s));
  // per block: known | status | state | rank | gidx | gflag | kc | cand_blk | cand_src | inc_base
  const size_t a8 = ix_al(n), a32 = ix_al(4 * n), a64 = ix_al(8 * n);
  HIPCHK(ctx, ix.acc.ensure(3 * a8 + 5 * a32 + 2 * a64));
  HIPCHK(ctx, ix.accv.ensure(2 * a64 + a8));
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(n)));
  char* b = ix.acc.as<char>();
  char* v = ix.accv.as<char>();
  const mvk::WgScan w = mvk::wg_scan_of(ix.wg.p, n);
  mvk::AcceptArrays a{};
  a.buf = d_buf, a.buf_bytes = buf_bytes, a.off = d_off, a.len = d_len, a.grp = d_grp, a.n = n;
  a.known = (uint8_t*)b, a.status = (uint8_t*)(b + a8), a.state = (uint8_t*)(b + 2 * a8);
  char* b32 = b + 3 * a8;
  a.rank = (uint32_t*)b32, a.gidx = (uint32_t*)(b32 + a32), a.gflag = (uint32_t*)(b32 + 2 * a32);
  a.kc = (uint32_t*)(b32 + 3 * a32), a.cand_blk = (uint32_t*)(b32 + 4 * a32);
  a.cand_src = (uint64_t*)(b32 + 5 * a32), a.inc_base = (uint64_t*)(b32 + 5 * a32 + a64);
  a.v_off = (uint64_t*)v, a.v_len = (uint64_t*)(v + a64), a.v_status = (uint8_t*)(v + 2 * a64);
  a.wg_a = w.count_a, a.wg_b = w.count_b, a.base_a = w.base_a, a.base_b = w.base_b;
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
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(ninc)));
  HIPCHK(ctx, ix.miss.ensure(48 * (size_t)capd + 8));
  HIPCHK(ctx, mvk::launch_accept_missing(table_of(ctx, ix), ix.item.as<uint64_t>(), ninc, ix.wg.as<uint64_t>(), ctl,
                                         ix.miss.as<uint64_t>(), capd, s));
  st = read_ctl(ctx, dev, s, &h);
  if (st != MV_OK) return st;
  out.n_missing = h[mvk::IX_CTL_NMISS];
  out.missing = ix.miss.as<uint64_t>();
  return MV_OK;
}

// the first device of the context, ready for an index call on its own stream
mv_status mvi::index_dev(mv_ctx* ctx, Device*& dev) {
  dev = &ctx->devs[0];
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  return order_behind_ahead(ctx, *dev, dev->stream);
}

// The host-buffer calls' way in: the blocks' bytes and the off | len | grp table go to the device,
// then accept_run.
mv_status mvi::stage_blocks(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
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

extern "C" {

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
  ix.dag.lin_marked = ix.dag.lin_height = 0;     // ... and the linearizer's marks
  if (ix.prop.on) {                              // ... and the proposer's queue, own block and choice
    st = propose_clear(ctx, *dev, dev->stream);
    if (st != MV_OK) return st;
  }
  if (!ix.slots) return MV_OK;
  if (ix.dag.on && ix.dag.map_slots) {
    HIPCHK(ctx, hipMemsetAsync(ix.dag.map.p, 0xff, 4 * (size_t)ix.dag.map_slots, dev->stream));
    HIPCHK(ctx, hipMemsetAsync(ix.dag.lmark.p, 0, 4 * (size_t)ix.dag.map_slots, dev->stream));
  }
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
  HIPCHK(ctx, ix.wg.ensure(mvk::wg_scan_bytes(ix.slots)));
  HIPCHK(ctx, ix.miss.ensure(48 * (size_t)capd + 8));
  uint64_t* ctl = ix.ctl.as<uint64_t>();
  HIPCHK(ctx, mvk::launch_index_wanted(table_of(ctx, ix), ix.wg.as<uint64_t>(), ctl + mvk::IX_CTL_NWANTED,
                                       ix.miss.as<uint64_t>(), capd, s));
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

}  // extern "C"
