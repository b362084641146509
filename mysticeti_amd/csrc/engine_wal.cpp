// libmysti_verify.so: the WAL calls -- the entry walk and crc check, the replay up to the block-store
// index on top of them, the write of new entries -- and the crc32 calls (they share the WAL path's
// crc tables).
#include <string.h>

#include <algorithm>

#include "engine_internal.h"
#include "wal_entry.h"
#include "wal_layout.h"

using namespace mvi;

extern "C" {

// ---------------------------------------------------------------- WAL replay
static mv_status wal_tables(mv_ctx* ctx, Device& dev) {
  if (dev.wal.tab.p) return MV_OK;
  std::vector<uint32_t> t(mvk::wal_table_words());
  mvk::wal_build_tables(t.data());
  HIPCHK(ctx, dev.wal.tab.ensure(4 * t.size()));
  HIPCHK(ctx, hipMemcpy(dev.wal.tab.p, t.data(), 4 * t.size(), hipMemcpyHostToDevice));
  if (!dev.cus) HIPCHK(ctx, hipDeviceGetAttribute(&dev.cus, hipDeviceAttributeMultiprocessorCount, dev.id));
  return MV_OK;
}

// Walk (one lane per map), join the maps in iteration order on the host, compact, crc pass.
static mv_status wal_run(mv_ctx* ctx, Device& dev, const uint8_t* d_img, uint64_t size, uint64_t end_pos,
                         uint32_t map_bits, uint64_t* d_pos, uint32_t* d_tag, uint32_t* d_len, uint8_t* d_status,
                         uint64_t cap, uint64_t* count, hipStream_t s) {
  *count = 0;
  mv_status st = wal_tables(ctx, dev);
  if (st != MV_OK) return st;
  const uint64_t msize = 1ull << map_bits, lim = std::min(size, end_pos);
  const uint64_t nmaps64 = (lim + msize - 1) >> map_bits;
  if (nmaps64 == 0) return MV_OK;
  if (nmaps64 > 0xffffffffull) return set_err(ctx, MV_E_INVALID_ARG, "too many maps");
  const uint32_t nmaps = (uint32_t)nmaps64;
  uint32_t cap_pm = (uint32_t)std::min<uint64_t>(msize / 16, 4096);
  std::vector<uint32_t> mcount(nmaps);
  std::vector<uint8_t> mflag(nmaps);
  uint32_t nincl = 0;
  uint64_t total = 0;
  mvr::EventSet ew, ec;  // stage timing: walk, crc
  if ((st = make_events(ctx, 1, ew)) != MV_OK || (st = make_events(ctx, 1, ec)) != MV_OK) return st;
  auto mark = [&](mvr::EventSet& e, int i) -> hipError_t {
    return e.empty() ? hipSuccess : hipEventRecord(e[i], s);
  };
  HIPCHK(ctx, dev.wal.rec.ensure(8 * (size_t)nmaps * cap_pm));
  HIPCHK(ctx, dev.wal.mcount.ensure(4 * (size_t)nmaps));
  HIPCHK(ctx, dev.wal.mflag.ensure(nmaps));
  HIPCHK(ctx, mark(ew, 0));
  HIPCHK(ctx, mvk::launch_wal_walk(d_img, size, end_pos, map_bits, nmaps, cap_pm, nullptr,
                                   dev.wal.rec.as<unsigned long long>(), dev.wal.mcount.as<uint32_t>(),
                                   dev.wal.mflag.as<uint8_t>(), s));
  HIPCHK(ctx, mark(ew, 1));
  HIPCHK(ctx, hipMemcpyAsync(mcount.data(), dev.wal.mcount.p, 4 * (size_t)nmaps, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(mflag.data(), dev.wal.mflag.p, nmaps, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  // WalIterator order: map after map while each one hands over to the next
  uint32_t maxc = 0;
  for (uint32_t m = 0; m < nmaps; m++) {
    if (mflag[m] == mvk::WAL_MAP_EMPTY) break;
    nincl = m + 1;
    total += mcount[m];
    maxc = std::max(maxc, mcount[m]);
    if (mflag[m] != mvk::WAL_MAP_NEXT) break;
  }
  keep_events(ctx, dev.id, kWalStage0, ew);
  if (total == 0) return MV_OK;
  std::vector<uint64_t> moff(nincl);
  for (uint64_t m = 0, o = 0; m < nincl; m++) {
    moff[m] = o;
    o += mcount[m];
  }
  HIPCHK(ctx, dev.wal.moff.ensure(8 * (size_t)nincl));
  HIPCHK(ctx, dev.wal.ent.ensure(8 * total));
  HIPCHK(ctx, dev.wal.ff.ensure(8));
  HIPCHK(ctx, hipMemcpyAsync(dev.wal.moff.p, moff.data(), 8 * (size_t)nincl, hipMemcpyHostToDevice, s));
  if (maxc <= cap_pm) {  // every map's records fit the first walk: compact them
    HIPCHK(ctx, mvk::launch_wal_compact(dev.wal.rec.as<unsigned long long>(), cap_pm, dev.wal.mcount.as<uint32_t>(),
                                        dev.wal.moff.as<uint64_t>(), nincl, dev.wal.ent.as<unsigned long long>(), s));
  } else {  // a map held more entries than the first guess: walk again straight into the entry list
    HIPCHK(ctx, mvk::launch_wal_walk(d_img, size, end_pos, map_bits, nincl, 0, dev.wal.moff.as<uint64_t>(),
                                     dev.wal.ent.as<unsigned long long>(), dev.wal.mcount.as<uint32_t>(),
                                     dev.wal.mflag.as<uint8_t>(), s));
  }
  HIPCHK(ctx, hipMemsetAsync(dev.wal.ff.p, 0xff, 8, s));
  HIPCHK(ctx, mark(ec, 0));
  HIPCHK(ctx, mvk::launch_wal_crc(d_img, size, dev.wal.ent.as<unsigned long long>(), total, dev.wal.tab.as<uint32_t>(),
                                  d_pos, d_tag, d_len, d_status, cap, dev.wal.ff.as<unsigned long long>(), dev.cus, s));
  HIPCHK(ctx, mark(ec, 1));
  keep_events(ctx, dev.id, kWalStage0 + 1, ec);
  uint64_t ff = 0;
  HIPCHK(ctx, hipMemcpyAsync(&ff, dev.wal.ff.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *count = ff < total ? ff + 1 : total;
  return MV_OK;
}

static bool wal_args_ok(uint32_t map_bits) { return map_bits >= 8 && map_bits <= 30; }

mv_status mv_wal_verify(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                        uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap,
                        uint64_t* count) {
  if (!ctx || !count || (size && !wal) || (cap && (!pos || !tag || !len || !status)) || !wal_args_ok(map_bits))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];  // one image, one device
  HIPCHK(ctx, hipSetDevice(dev.id));
  hipStream_t s = dev.stream;
  HIPCHK(ctx, dev.wal.img.ensure(size + 16));
  if (size) HIPCHK(ctx, hipMemcpyAsync(dev.wal.img.p, wal, size, hipMemcpyHostToDevice, s));
  // outputs: device arrays of up to cap entries; the walk bounds the entry count by size / 16
  const uint64_t ocap = std::min<uint64_t>(cap, size / 16 + 1);
  HIPCHK(ctx, dev.wal.pos.ensure(8 * ocap + 8));
  HIPCHK(ctx, dev.wal.tag.ensure(4 * ocap + 4));
  HIPCHK(ctx, dev.wal.len.ensure(4 * ocap + 4));
  HIPCHK(ctx, dev.wal.st.ensure(ocap + 1));
  uint64_t n = 0;
  mv_status st = wal_run(ctx, dev, dev.wal.img.as<uint8_t>(), size, end_pos, map_bits, dev.wal.pos.as<uint64_t>(),
                         dev.wal.tag.as<uint32_t>(), dev.wal.len.as<uint32_t>(), dev.wal.st.as<uint8_t>(), ocap, &n, s);
  if (st != MV_OK) return st;
  const uint64_t w = std::min(n, ocap);
  if (w) {
    HIPCHK(ctx, hipMemcpyAsync(pos, dev.wal.pos.p, 8 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(tag, dev.wal.tag.p, 4 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(len, dev.wal.len.p, 4 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(status, dev.wal.st.p, w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  *count = n;
  return MV_OK;
}

mv_status mv_dev_wal_verify(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size, uint64_t end_pos,
                            uint32_t map_bits, uint64_t* d_pos, uint32_t* d_tag, uint32_t* d_len, uint8_t* d_status,
                            uint64_t cap, uint64_t* count, void* stream) {
  if (!ctx || !count || (size && !d_wal) || (cap && (!d_pos || !d_tag || !d_len || !d_status)) ||
      !wal_args_ok(map_bits))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal args");
  if (((uintptr_t)d_wal) & 3) return set_err(ctx, MV_E_INVALID_ARG, "d_wal must be 4-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  return wal_run(ctx, *dev, d_wal, size, end_pos, map_bits, d_pos, d_tag, d_len, d_status, cap, count, s);
}

// ---------------------------------------------------------------- WAL replay up to the index
namespace {
constexpr size_t rp_al(size_t x) { return (x + 255) & ~(size_t)255; }

// Where replay_run leaves its results (device memory of dev.wal)
struct ReplayOut {
  uint64_t count = 0, n_rows = 0;
  const uint64_t* pos = nullptr;
  const uint32_t *tag = nullptr, *len = nullptr;
  const uint8_t* st = nullptr;
  const uint64_t* rows = nullptr;
  const uint8_t* blk_status = nullptr;
};

// wal_run into the device's own entry arrays, then the replay kernels and the block pipeline on
// the blocks they list (in place in d_img), on stream s. d_summary (3) and d_last_seen (committee
// size) are written on the device. Synchronises s: wal_run does, the block count sizes the
// pipeline's launches, and the two counts end the call.
mv_status replay_run(mv_ctx* ctx, Device& dev, const uint8_t* d_img, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                     uint64_t* d_summary, uint64_t* d_last_seen, hipStream_t s, ReplayOut& out) {
  out = ReplayOut();
  const uint32_t n_auth = ctx->committee.size();
  // the walk bounds the entry count by size / 16
  const uint64_t ocap = size / 16 + 1;
  HIPCHK(ctx, dev.wal.pos.ensure(8 * ocap + 8));
  HIPCHK(ctx, dev.wal.tag.ensure(4 * ocap + 4));
  HIPCHK(ctx, dev.wal.len.ensure(4 * ocap + 4));
  HIPCHK(ctx, dev.wal.st.ensure(ocap + 1));
  uint64_t n = 0;
  mv_status st = wal_run(ctx, dev, d_img, size, end_pos, map_bits, dev.wal.pos.as<uint64_t>(), dev.wal.tag.as<uint32_t>(),
                         dev.wal.len.as<uint32_t>(), dev.wal.st.as<uint8_t>(), ocap, &n, s);
  if (st != MV_OK) return st;
  n = std::min(n, ocap);
  // control words | counts
  HIPCHK(ctx, dev.wal.rctl.ensure(8 * (mvk::REPLAY_CTL_WORDS + 2)));
  uint64_t* ctl = dev.wal.rctl.as<uint64_t>();
  uint64_t* counts = ctl + mvk::REPLAY_CTL_WORDS;
  HIPCHK(ctx, hipMemsetAsync(ctl, 0, 8 * (mvk::REPLAY_CTL_WORDS + 2), s));
  HIPCHK(ctx, hipMemsetAsync(ctl + mvk::REPLAY_CTL_FF, 0xff, 8, s));
  HIPCHK(ctx, hipMemsetAsync(d_last_seen, 0, 8 * (size_t)n_auth, s));
  const mvk::ReplayEntries en{dev.wal.pos.as<uint64_t>(), dev.wal.tag.as<uint32_t>(), dev.wal.len.as<uint32_t>(),
                              dev.wal.st.as<uint8_t>(), n};
  mvk::ReplayBlocks bl{};
  if (n) {
    // per workgroup: count | base; per entry (the lists' bound): off | len | ent | block status
    const size_t nwg = mvk::replay_groups(n), a64 = rp_al(8 * n);
    const size_t o_base = rp_al(8 * nwg), o_list = o_base + rp_al(8 * nwg);
    HIPCHK(ctx, dev.wal.rscr.ensure(o_list + 3 * a64 + rp_al(n)));
    char* b = dev.wal.rscr.as<char>();
    uint64_t* wgbase = (uint64_t*)(b + o_base);
    bl = mvk::ReplayBlocks{(uint64_t*)(b + o_list), (uint64_t*)(b + o_list + a64), (uint64_t*)(b + o_list + 2 * a64),
                           (uint8_t*)(b + o_list + 3 * a64), 0, n};
    HIPCHK(ctx, mvk::launch_replay_select(en, size, (uint64_t*)b, wgbase, ctl + mvk::REPLAY_CTL_NB, s));
    uint64_t nb = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nb, ctl + mvk::REPLAY_CTL_NB, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    bl.n = std::min(nb, n);
    if (bl.n) {
      HIPCHK(ctx, mvk::launch_replay_list(en, size, wgbase, bl, s));
      HIPCHK(ctx, dev.wal.rows.ensure(8 * (size_t)mv::we::ROW_WORDS * bl.n));
      // the block path as mv_dev_verify_blocks runs it, in chunks of at most max_batch blocks
      for (uint64_t i = 0; i < bl.n;) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(bl.n - i, ctx->max_batch);
        st = enqueue_blocks(ctx, dev, d_img, size, bl.off + i, bl.len + i, m, bl.status + i, nullptr, nullptr, s);
        if (st != MV_OK) {
          (void)hipStreamSynchronize(s);
          return st;
        }
        i += m;
      }
      HIPCHK(ctx, mvk::launch_replay_rows(d_img, en, bl, n_auth, dev.wal.rows.as<uint64_t>(), s));
    }
  }
  HIPCHK(ctx, mvk::launch_replay_summary(en, bl, dev.wal.rows.as<uint64_t>(), n_auth, ctl, d_summary, d_last_seen,
                                         counts, s));
  uint64_t h_counts[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h_counts, counts, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  poll_flags(ctx, dev);
  out.count = std::min(h_counts[0], n);
  out.n_rows = std::min(h_counts[1], bl.n);
  out.pos = en.pos;
  out.tag = en.tag;
  out.len = en.len;
  out.st = en.status;
  out.rows = dev.wal.rows.as<uint64_t>();
  out.blk_status = bl.status;
  return MV_OK;
}

bool replay_args_ok(const void* img, uint64_t size, uint32_t map_bits, const void* pos, const void* tag, const void* len,
                    const void* status, uint64_t cap, const void* count, const void* rows, uint64_t cap_blocks,
                    const void* n_blocks, const void* summary, const void* last_seen) {
  return count && n_blocks && summary && last_seen && !(size && !img) && !(cap && (!pos || !tag || !len || !status)) &&
         !(cap_blocks && !rows) && wal_args_ok(map_bits);
}
}  // namespace

// mv_wal_replay, and with `seeded` mv_wal_recover: the same replay, then one seed call over all its
// rows while image, rows and verdicts are still in the device's own buffers
static mv_status wal_replay_host(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                                 uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap, uint64_t* count,
                                 uint64_t* blk_rows, uint8_t* blk_status, uint64_t cap_blocks, uint64_t* n_blocks,
                                 uint64_t* summary, uint64_t* last_seen, uint64_t floor_round, uint64_t* seeded) {
  if (!ctx || !replay_args_ok(wal, size, map_bits, pos, tag, len, status, cap, count, blk_rows, cap_blocks, n_blocks,
                              summary, last_seen))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal replay args");
  *count = 0;
  *n_blocks = 0;
  if (seeded) memset(seeded, 0, 5 * sizeof(uint64_t));
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device& dev = ctx->devs[0];  // one image, one device
  if (seeded && !dev.index.dag.on) return set_err(ctx, MV_E_INVALID_ARG, "mv_dag_reserve first");
  HIPCHK(ctx, hipSetDevice(dev.id));
  reap_idle(ctx, dev);
  hipStream_t s = dev.stream;
  const uint32_t n_auth = ctx->committee.size();
  HIPCHK(ctx, dev.wal.img.ensure(size + 16));
  if (size) HIPCHK(ctx, hipMemcpyAsync(dev.wal.img.p, wal, size, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemsetAsync(dev.wal.img.as<uint8_t>() + size, 0, 16, s));  // the readable bytes past the last block
  HIPCHK(ctx, dev.wal.rsum.ensure(8 * (3 + (size_t)n_auth)));
  uint64_t* d_summary = dev.wal.rsum.as<uint64_t>();
  ReplayOut ro;
  const mv_status st = replay_run(ctx, dev, dev.wal.img.as<uint8_t>(), size, end_pos, map_bits, d_summary, d_summary + 3,
                                  s, ro);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);  // (the image copy may still be in flight)
    return st;
  }
  const uint64_t w = std::min(ro.count, cap), wr = std::min(ro.n_rows, cap_blocks);
  if (w) {
    HIPCHK(ctx, hipMemcpyAsync(pos, ro.pos, 8 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(tag, ro.tag, 4 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(len, ro.len, 4 * w, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(status, ro.st, w, hipMemcpyDeviceToHost, s));
  }
  if (wr) {
    HIPCHK(ctx, hipMemcpyAsync(blk_rows, ro.rows, 8 * (size_t)mv::we::ROW_WORDS * wr, hipMemcpyDeviceToHost, s));
    if (blk_status) HIPCHK(ctx, hipMemcpyAsync(blk_status, ro.blk_status, wr, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ctx, hipMemcpyAsync(summary, d_summary, 24, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(last_seen, d_summary + 3, 8 * (size_t)n_auth, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *count = ro.count;
  *n_blocks = ro.n_rows;
  if (!seeded) return MV_OK;
  const mv_status sd = dag_seed_run(ctx, dev, dev.wal.img.as<uint8_t>(), size, ro.rows, ro.blk_status, ro.n_rows, floor_round,
                                    /*can_grow=*/true, s, seeded);
  if (sd != MV_OK) (void)hipStreamSynchronize(s);
  return sd;
}

mv_status mv_wal_replay(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                        uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap, uint64_t* count,
                        uint64_t* blk_rows, uint8_t* blk_status, uint64_t cap_blocks, uint64_t* n_blocks,
                        uint64_t* summary, uint64_t* last_seen) {
  return wal_replay_host(ctx, wal, size, end_pos, map_bits, pos, tag, len, status, cap, count, blk_rows, blk_status,
                         cap_blocks, n_blocks, summary, last_seen, 0, nullptr);
}

mv_status mv_wal_recover(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                         uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap, uint64_t* count,
                         uint64_t* blk_rows, uint8_t* blk_status, uint64_t cap_blocks, uint64_t* n_blocks,
                         uint64_t* summary, uint64_t* last_seen, uint64_t floor_round, uint64_t* seeded) {
  if (!seeded) return set_err(ctx, MV_E_INVALID_ARG, "bad wal recover args");
  return wal_replay_host(ctx, wal, size, end_pos, map_bits, pos, tag, len, status, cap, count, blk_rows, blk_status,
                         cap_blocks, n_blocks, summary, last_seen, floor_round, seeded);
}

mv_status mv_dev_wal_replay(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size, uint64_t end_pos,
                            uint32_t map_bits, uint64_t* d_pos, uint32_t* d_tag, uint32_t* d_len, uint8_t* d_status,
                            uint64_t cap, uint64_t* count, uint64_t* d_blk_rows, uint8_t* d_blk_status,
                            uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* d_summary, uint64_t* d_last_seen,
                            void* stream) {
  if (!ctx || !replay_args_ok(d_wal, size, map_bits, d_pos, d_tag, d_len, d_status, cap, count, d_blk_rows, cap_blocks,
                              n_blocks, d_summary, d_last_seen))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal replay args");
  if (((uintptr_t)d_wal) & 7) return set_err(ctx, MV_E_INVALID_ARG, "d_wal must be 8-byte aligned");
  *count = 0;
  *n_blocks = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  ReplayOut ro;
  const mv_status st = replay_run(ctx, *dev, d_wal, size, end_pos, map_bits, d_summary, d_last_seen, s, ro);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  const uint64_t w = std::min(ro.count, cap), wr = std::min(ro.n_rows, cap_blocks);
  if (w) {
    HIPCHK(ctx, hipMemcpyAsync(d_pos, ro.pos, 8 * w, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_tag, ro.tag, 4 * w, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_len, ro.len, 4 * w, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_status, ro.st, w, hipMemcpyDeviceToDevice, s));
  }
  if (wr) {
    HIPCHK(ctx, hipMemcpyAsync(d_blk_rows, ro.rows, 8 * (size_t)mv::we::ROW_WORDS * wr, hipMemcpyDeviceToDevice, s));
    if (d_blk_status) HIPCHK(ctx, hipMemcpyAsync(d_blk_status, ro.blk_status, wr, hipMemcpyDeviceToDevice, s));
  }
  if (w || wr) HIPCHK(ctx, hipStreamSynchronize(s));
  *count = ro.count;
  *n_blocks = ro.n_rows;
  return MV_OK;
}

uint64_t mv_wal_layout(const uint64_t* payload_len, uint64_t n, uint32_t map_bits, uint64_t start, uint64_t* pos) {
  if (!wal_args_ok(map_bits) || (n && (!payload_len || !pos))) return start;
  uint64_t p = start;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t len = payload_len[i] + mv::wl::HEADER;  // header + payload (wal.rs:152)
    p = mv::wl::entry_pos(p, len, map_bits);               // zero padding (wal.rs:163-167)
    pos[i] = p;
    p += len;
  }
  return p;
}

// ---------------------------------------------------------------- WAL write
namespace {
constexpr uint64_t kMaxWalEntries = 0xffffffffull;

bool wal_write_args_ok(const void* buf, uint64_t buf_bytes, const void* entries, uint64_t n, uint64_t start,
                       uint32_t map_bits, const void* out, uint64_t cap, const void* pos, const void* end_pos) {
  return end_pos && wal_args_ok(map_bits) && !(buf_bytes && !buf) && !(n && (!entries || !pos)) && !(cap && !out) &&
         n <= kMaxWalEntries && start <= (1ull << 62) && buf_bytes <= ~0ull - 64 && cap <= ~0ull - 64;
}

// One call on device arrays (c: the caller's, the scratch is filled in here), on stream s: the
// layout, its control words read back (the one synchronise), then -- if nothing was refused and the
// span fits cap -- the bytes, enqueued. *end_pos = c.start where the call is refused.
mv_status wal_write_run(mv_ctx* ctx, Device& dev, mvk::WalWriteCall c, hipStream_t s, uint64_t* end_pos) {
  *end_pos = c.start;
  if (c.n == 0) return MV_OK;
  mv_status st = wal_tables(ctx, dev);
  if (st != MV_OK) return st;
  Device::Wal& q = dev.wal;
  const bool fresh = !q.wctl.p;
  HIPCHK(ctx, q.wctl.ensure(8 * mvk::WW_CTL_WORDS));
  HIPCHK(ctx, q.wsum.ensure(8 * c.n));
  HIPCHK(ctx, q.wcross.ensure(16 * c.n));
  HIPCHK(ctx, q.wwg.ensure(mvk::wg_scan_bytes(c.n)));
  c.sums = q.wsum.as<uint64_t>();
  c.cross_first = q.wcross.as<uint64_t>();
  c.cross_shift = c.cross_first + c.n;
  uint64_t* ctl = q.wctl.as<uint64_t>();
  // (the byte pass's error word outlives a call: it is reported by the next one)
  HIPCHK(ctx, hipMemsetAsync(ctl, 0, fresh ? 8 * mvk::WW_CTL_WORDS : 8 * mvk::WW_CTL_ERR, s));
  HIPCHK(ctx, mvk::launch_wal_write_layout(c, q.wwg.p, ctl, s));
  uint64_t w[mvk::WW_CTL_WORDS] = {0};
  HIPCHK(ctx, hipMemcpyAsync(w, ctl, sizeof w, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (w[mvk::WW_CTL_ERR]) {
    HIPCHK(ctx, hipMemsetAsync(ctl + mvk::WW_CTL_ERR, 0, 8, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return set_err(ctx, MV_E_HIP, "wal write: a bounds check failed on the device");
  }
  if (w[mvk::WW_CTL_BAD])
    return set_err(ctx, MV_E_INVALID_ARG, "wal write: a payload leaves buf or a body is longer than a map holds");
  *end_pos = w[mvk::WW_CTL_END];
  if (*end_pos - c.start > c.cap) return MV_OK;  // pos and *end_pos are written, no byte of out
  HIPCHK(ctx, mvk::launch_wal_write_emit(c, q.tab.as<uint32_t>(), ctl, dev.cus, s));
  return MV_OK;
}
}  // namespace

mv_status mv_wal_write(mv_ctx* ctx, const uint8_t* buf, uint64_t buf_bytes, const uint64_t* entries, uint64_t n,
                       uint64_t start, uint32_t map_bits, uint8_t* out, uint64_t cap, uint64_t* pos, uint64_t* end_pos) {
  if (!ctx || !wal_write_args_ok(buf, buf_bytes, entries, n, start, map_bits, out, cap, pos, end_pos))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal write args");
  *end_pos = start;
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  Device::Wal& q = dev.wal;
  HIPCHK(ctx, hipSetDevice(dev.id));
  hipStream_t s = dev.stream;
  HIPCHK(ctx, q.wbuf.ensure(buf_bytes + 16));
  HIPCHK(ctx, q.went.ensure(8 * (size_t)mv::wl::ENTRY_WORDS * n));
  HIPCHK(ctx, q.wpos.ensure(8 * n));
  if (buf_bytes) HIPCHK(ctx, hipMemcpyAsync(q.wbuf.p, buf, buf_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemsetAsync(q.wbuf.as<uint8_t>() + buf_bytes, 0, 16, s));  // (payloads are read as whole aligned words)
  HIPCHK(ctx, hipMemcpyAsync(q.went.p, entries, 8 * (size_t)mv::wl::ENTRY_WORDS * n, hipMemcpyHostToDevice, s));
  mvk::WalWriteCall c{};
  c.buf = q.wbuf.as<uint8_t>(), c.buf_bytes = buf_bytes;
  c.entries = q.went.as<uint64_t>(), c.n = n;
  c.start = start, c.map_bits = map_bits;
  c.out = nullptr, c.cap = 0;  // the layout first: the image is sized by what it says
  c.pos = q.wpos.as<uint64_t>();
  uint64_t end = start;
  mv_status rc = wal_write_run(ctx, dev, c, s, &end);
  if (rc != MV_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  const uint64_t span = end - start;
  if (span && span <= cap) {
    HIPCHK(ctx, q.wout.ensure(span + 16));
    c.out = q.wout.as<uint8_t>(), c.cap = span;
    HIPCHK(ctx, mvk::launch_wal_write_emit(c, q.tab.as<uint32_t>(), q.wctl.as<uint64_t>(), dev.cus, s));
    HIPCHK(ctx, hipMemcpyAsync(out, c.out, span, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ctx, hipMemcpyAsync(pos, c.pos, 8 * n, hipMemcpyDeviceToHost, s));
  uint64_t err = 0;
  HIPCHK(ctx, hipMemcpyAsync(&err, q.wctl.as<uint64_t>() + mvk::WW_CTL_ERR, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  *end_pos = end;
  if (err) {
    HIPCHK(ctx, hipMemsetAsync(q.wctl.as<uint64_t>() + mvk::WW_CTL_ERR, 0, 8, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return set_err(ctx, MV_E_HIP, "wal write: a bounds check failed on the device");
  }
  return MV_OK;
}

mv_status mv_dev_wal_write(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_entries,
                           uint64_t n, uint64_t start, uint32_t map_bits, uint8_t* d_out, uint64_t cap, uint64_t* d_pos,
                           uint64_t* end_pos, void* stream) {
  if (!ctx || !wal_write_args_ok(d_buf, buf_bytes, d_entries, n, start, map_bits, d_out, cap, d_pos, end_pos))
    return set_err(ctx, MV_E_INVALID_ARG, "bad wal write args");
  if (((uintptr_t)d_buf | (uintptr_t)d_entries | (uintptr_t)d_out | (uintptr_t)d_pos) & 7)
    return set_err(ctx, MV_E_INVALID_ARG, "wal write: misaligned device pointer");
  *end_pos = start;
  if (n == 0) return MV_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev || dev != &ctx->devs[0]) return set_err(ctx, MV_E_NO_DEVICE, "wal write runs on the context's first device");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)dev->stream;
  mvk::WalWriteCall c{};
  c.buf = d_buf, c.buf_bytes = buf_bytes;
  c.entries = d_entries, c.n = n;
  c.start = start, c.map_bits = map_bits;
  c.out = d_out, c.cap = cap;
  c.pos = d_pos;
  return wal_write_run(ctx, *dev, c, s, end_pos);
}

mv_status mv_crc32(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                   uint32_t* out) {
  if (!ctx || (n && (!buf || !off || !len || !out))) return set_err(ctx, MV_E_INVALID_ARG, "bad crc32 args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  return for_each_shard(ctx, n, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
    HIPCHK(ctx, hipSetDevice(dev.id));
    mv_status st = wal_tables(ctx, dev);
    if (st != MV_OK) return st;
    uint64_t i = lo;
    while (i < hi) {
      uint64_t j = i, bytes = 0;  // chunks of <= max_batch strings and <= 1 GiB
      while (j < hi && j - i < ctx->max_batch && bytes < (1ull << 30)) bytes += len[j++];
      const uint32_t m = (uint32_t)(j - i);
      HIPCHK(ctx, dev.hc.h_in.ensure(bytes + 16));
      uint8_t* stg = dev.hc.h_in.as<uint8_t>();
      std::vector<uint64_t> soff(m), slen(m);
      uint64_t p = 0;
      for (uint32_t k = 0; k < m; k++) {
        soff[k] = p;
        slen[k] = len[i + k];
        memcpy(stg + p, buf + off[i + k], slen[k]);
        p += slen[k];
      }
      HIPCHK(ctx, dev.hc.bytes.ensure(p + 16));
      HIPCHK(ctx, dev.hc.off.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.len.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.out2.ensure(4 * (size_t)m));
      if (p) HIPCHK(ctx, hipMemcpyAsync(dev.hc.bytes.p, stg, p, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.off.p, soff.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.len.p, slen.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, mvk::launch_crc32(dev.hc.bytes.as<uint8_t>(), dev.hc.off.as<uint64_t>(), dev.hc.len.as<uint64_t>(), m,
                                    dev.wal.tab.as<uint32_t>(), dev.hc.out2.as<uint32_t>(), dev.cus, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(out + i, dev.hc.out2.p, 4 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipStreamSynchronize(dev.stream));
      i = j;
    }
    return MV_OK;
  });
}

mv_status mv_dev_crc32(mv_ctx* ctx, int device, const uint8_t* d_buf, const uint64_t* d_off, const uint64_t* d_len,
                       uint32_t n, uint32_t* d_out, void* stream) {
  if (!ctx || (n && (!d_buf || !d_off || !d_len || !d_out))) return set_err(ctx, MV_E_INVALID_ARG, "bad args");
  if (((uintptr_t)d_buf) & 3) return set_err(ctx, MV_E_INVALID_ARG, "d_buf must be 4-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  mv_status st = wal_tables(ctx, *dev);
  if (st != MV_OK) return st;
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  HIPCHK(ctx, mvk::launch_crc32(d_buf, d_off, d_len, n, dev->wal.tab.as<uint32_t>(), d_out, dev->cus, s));
  return MV_OK;
}

}  // extern "C"
