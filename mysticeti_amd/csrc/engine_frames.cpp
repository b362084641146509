// libmysti_verify.so: received frames -- the host statement of the walk and mv_verify_frames.
#include <string.h>

#include <algorithm>

#include "engine_internal.h"
#include "frame_walk.h"

using namespace mvi;

extern "C" {

// ---------------------------------------------------------------- frames with message verdicts
// The CPU statement of the walk mv_verify_frames runs on the device (frame_walk.h holds the
// rules for both): one stream, the statuses the bytes alone decide.
int64_t mv_frame_messages(const uint8_t* buf, uint64_t len, uint32_t* msgs, uint64_t cap_msgs, uint64_t* blk_off,
                          uint64_t* blk_len, uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* consumed) {
  namespace fr = mv::fr;
  if (consumed) *consumed = 0;
  if (n_blocks) *n_blocks = 0;
  if ((len && !buf) || (cap_msgs && !msgs) || (cap_blocks && (!blk_off || !blk_len))) return -1;
  struct Sink {
    uint64_t *off, *len, first, cap;
    void operator()(uint32_t k, uint64_t o, uint64_t l) const {
      if (first + k < cap) {
        off[first + k] = o;
        len[first + k] = l;
      }
    }
  };
  uint64_t p = 0, rows = 0, found = 0;
  for (;;) {
    uint64_t size;
    const fr::Step st = fr::frame_at(buf, p, len, size);
    if (st == fr::STEP_END) break;
    if (st == fr::STEP_PING) {
      p += 4 + fr::PING_REST;
      if (consumed) *consumed = p;
      continue;
    }
    fr::Msg m{fr::NO_TAG, MV_MSG_BAD_SIZE, 0};
    if (st == fr::STEP_FRAME) m = fr::classify(buf, p + 4, size, Sink{blk_off, blk_len, found, cap_blocks});
    if (found + m.nblk > 0xffffffffull || rows >= 0xffffffffull) return -1;  // rows hold 32-bit indices
    if (rows < cap_msgs)
      fr::put_row(msgs + fr::ROW_WORDS * rows, 0, m.tag, p, (uint32_t)found, m.nblk, m.status, 0, fr::NONE);
    rows++;
    found += m.nblk;
    if (st == fr::STEP_BAD_SIZE) break;  // consumed ends before the frame
    p += 4 + size;
    if (consumed) *consumed = p;
    if (m.status != MV_MSG_OK) break;
  }
  if (n_blocks) *n_blocks = found;
  return (int64_t)rows;
}

namespace {
constexpr size_t frm_al(size_t x) { return (x + 255) & ~(size_t)255; }

// Where frames_run leaves its results (device memory of dev.frm.s / dev.frm.o)
struct FramesOut {
  uint64_t n_rows = 0, n_blk = 0;
  uint32_t* rows = nullptr;
  uint64_t *blk_off = nullptr, *blk_len = nullptr, *consumed = nullptr;
  uint8_t* blk_status = nullptr;
  uint32_t* drop = nullptr;
  // host sides of the scans: sources of copies enqueued by frames_run, alive until the caller's sync
  std::vector<uint32_t> h32, hb32;
  std::vector<uint64_t> h64;
};

// The device walk, the block pipeline on the blocks it lists (in place in d_buf) and the
// verdicts, on stream s. Synchronises s twice on the way (the frame and the row / block counts
// size the lists); the last kernels are enqueued only.
mv_status frames_run(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_soff,
                     const uint64_t* d_slen, uint32_t ns, hipStream_t s, FramesOut& out) {
  const size_t n = ns;
  // per stream: fcount | kept | row_base | blk_base | drop | foff | sblocks | consumed
  const size_t a32 = frm_al(4 * n), a64 = frm_al(8 * n);
  HIPCHK(ctx, dev.frm.s.ensure(5 * a32 + 3 * a64));
  char* b = dev.frm.s.as<char>();
  uint32_t* fcount = (uint32_t*)b;
  uint32_t* kept = (uint32_t*)(b + a32);
  uint32_t* row_base = (uint32_t*)(b + 2 * a32);
  uint32_t* blk_base = (uint32_t*)(b + 3 * a32);
  uint32_t* drop = (uint32_t*)(b + 4 * a32);
  uint64_t* foff = (uint64_t*)(b + 5 * a32);
  uint64_t* sblocks = (uint64_t*)(b + 5 * a32 + a64);
  uint64_t* consumed = (uint64_t*)(b + 5 * a32 + 2 * a64);
  out = FramesOut();
  out.consumed = consumed;
  out.drop = drop;
  std::vector<uint32_t>&h32 = out.h32, &hb32 = out.hb32;
  std::vector<uint64_t>& h64 = out.h64;
  h32.assign(n, 0);
  hb32.assign(n, 0);
  h64.assign(n, 0);
  HIPCHK(ctx, mvk::launch_frame_walk(d_buf, buf_bytes, d_soff, d_slen, ns, nullptr, nullptr, nullptr, nullptr, fcount,
                                     consumed, s));
  HIPCHK(ctx, hipMemcpyAsync(h32.data(), fcount, 4 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  uint64_t nf = 0;
  for (size_t k = 0; k < n; k++) {
    h64[k] = nf;
    nf += h32[k];
  }
  HIPCHK(ctx, hipMemsetAsync(kept, 0, 3 * a32, s));  // kept, row_base, blk_base (no frames: no rows)
  mvk::FrameList fl{};
  uint64_t* bpre = nullptr;
  if (nf) {
    // per frame: off | bpre | size | stream | tag | nblk | status
    const size_t f64 = frm_al(8 * nf), f32 = frm_al(4 * nf);
    HIPCHK(ctx, dev.frm.f.ensure(2 * f64 + 4 * f32 + frm_al(nf)));
    char* f = dev.frm.f.as<char>();
    uint64_t* fr_off = (uint64_t*)f;
    bpre = (uint64_t*)(f + f64);
    uint32_t* fr_size = (uint32_t*)(f + 2 * f64);
    uint32_t* fr_stream = (uint32_t*)(f + 2 * f64 + f32);
    fl = mvk::FrameList{fr_off, fr_size, fr_stream, nf, (uint32_t*)(f + 2 * f64 + 2 * f32),
                        (uint8_t*)(f + 2 * f64 + 4 * f32), (uint32_t*)(f + 2 * f64 + 3 * f32)};
    HIPCHK(ctx, hipMemcpyAsync(foff, h64.data(), 8 * n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, mvk::launch_frame_walk(d_buf, buf_bytes, d_soff, d_slen, ns, foff, fr_off, fr_size, fr_stream, fcount,
                                       consumed, s));
    HIPCHK(ctx, mvk::launch_msg_walk(d_buf, fl, nullptr, s));
    HIPCHK(ctx, mvk::launch_stream_cut(d_soff, buf_bytes, ns, fcount, foff, fl, bpre, kept, sblocks, consumed, s));
    HIPCHK(ctx, hipMemcpyAsync(h32.data(), kept, 4 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h64.data(), sblocks, 8 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    uint64_t nr = 0, nb = 0;
    for (size_t k = 0; k < n; k++) {
      const uint64_t r = h32[k], bl = h64[k];
      h32[k] = (uint32_t)nr;
      hb32[k] = (uint32_t)nb;
      nr += r;
      nb += bl;
      if (nr > 0xffffffffull || nb > 0xffffffffull)
        return set_err(ctx, MV_E_INVALID_ARG, "more than 2^32 messages or blocks in one call");
    }
    out.n_rows = nr;
    out.n_blk = nb;
    HIPCHK(ctx, hipMemcpyAsync(row_base, h32.data(), 4 * n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(blk_base, hb32.data(), 4 * n, hipMemcpyHostToDevice, s));
  }
  // rows | blk_off | blk_len | blk_status
  const size_t o_rows = frm_al(32 * (size_t)out.n_rows), o_b64 = frm_al(8 * (size_t)out.n_blk);
  HIPCHK(ctx, dev.frm.o.ensure(o_rows + 2 * o_b64 + frm_al(out.n_blk) + 256));
  char* o = dev.frm.o.as<char>();
  out.rows = (uint32_t*)o;
  out.blk_off = (uint64_t*)(o + o_rows);
  out.blk_len = (uint64_t*)(o + o_rows + o_b64);
  out.blk_status = (uint8_t*)(o + o_rows + 2 * o_b64);
  if (out.n_rows) {
    // (zeroed lists: an entry the second walk does not write is an empty block, never a stray offset)
    if (out.n_blk) HIPCHK(ctx, hipMemsetAsync(out.blk_off, 0, 2 * o_b64, s));
    const mvk::FrameRows fr{foff, kept, row_base, blk_base, bpre, out.rows, out.n_rows, out.blk_off, out.blk_len, out.n_blk};
    HIPCHK(ctx, mvk::launch_msg_walk(d_buf, fl, &fr, s));
  }
  // the block path as mv_dev_verify_blocks runs it, in chunks of at most max_batch blocks
  for (uint64_t i = 0; i < out.n_blk;) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(out.n_blk - i, ctx->max_batch);
    const mv_status st = enqueue_blocks(ctx, dev, d_buf, buf_bytes, out.blk_off + i, out.blk_len + i, m,
                                        out.blk_status + i, nullptr, nullptr, s);
    if (st != MV_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
    i += m;
  }
  HIPCHK(ctx, mvk::launch_frame_verdicts(out.rows, out.n_rows, out.blk_status, out.n_blk, ns, kept, row_base, drop, s));
  return MV_OK;
}

// One shard's results on the host, before the merge rebases them
struct FrameShard {
  uint64_t lo = 0, hi = 0, n_rows = 0, n_blk = 0;
  std::vector<uint32_t> rows;
  std::vector<uint64_t> blk_off, blk_len, delta;  // delta[k]: caller offset - device offset of stream lo + k
  std::vector<uint8_t> blk_status;
};

// Streams [lo, hi) of a host-buffer call on dev: their bytes to the device (pinned, in order
// and disjoint: one DMA of the caller's memory in place; else packed stream by stream, which
// also separates overlapping streams), the walk, the results back.
mv_status frames_shard(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* soff, const uint64_t* slen,
                       uint64_t* consumed, uint32_t* drop_msg, FrameShard& sh) {
  HIPCHK(ctx, hipSetDevice(dev.id));
  reap_idle(ctx, dev);
  hipStream_t s = dev.stream;
  const uint64_t lo = sh.lo, ns = sh.hi - sh.lo;
  uint64_t bytes = 0, span = 0;
  const uint64_t first = soff[lo];
  bool direct = host_pinned(buf + first);
  for (uint64_t k = lo; k < sh.hi; k++) {
    bytes += (slen[k] + 7) & ~7ull;
    if (direct && (soff[k] < first || soff[k] - first < span)) direct = false;  // in order, disjoint
    if (direct) span = soff[k] - first + slen[k];
  }
  direct = direct && span && span <= 2 * bytes + 4096 && pinned_range_holds(buf + first, span);
  const uint64_t buf_bytes = direct ? span : bytes;
  std::vector<uint64_t> tab(2 * ns);  // device offsets | lengths
  sh.delta.resize(ns);
  HIPCHK(ctx, dev.frm.in.ensure(buf_bytes + 32));
  uint8_t* d_buf = dev.frm.in.as<uint8_t>();
  if (direct) {
    for (uint64_t k = 0; k < ns; k++) {
      tab[k] = soff[lo + k] - first;
      tab[ns + k] = slen[lo + k];
      sh.delta[k] = first;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_buf, buf + first, span, hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(ctx, dev.hc.h_in.ensure(bytes + 32));
    uint8_t* h = dev.hc.h_in.as<uint8_t>();
    uint64_t p = 0;
    for (uint64_t k = 0; k < ns; k++) {
      const uint64_t l = slen[lo + k], pl = (l + 7) & ~7ull;
      if (l) memcpy(h + p, buf + soff[lo + k], l);
      memset(h + p + l, 0, pl - l);
      tab[k] = p;
      tab[ns + k] = l;
      sh.delta[k] = soff[lo + k] - p;
      p += pl;
    }
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(d_buf, h, bytes, hipMemcpyHostToDevice, s));
  }
  HIPCHK(ctx, hipMemsetAsync(d_buf + buf_bytes, 0, 32, s));  // the readable bytes past the last block
  HIPCHK(ctx, dev.frm.tab.ensure(16 * ns));
  HIPCHK(ctx, hipMemcpyAsync(dev.frm.tab.p, tab.data(), 16 * ns, hipMemcpyHostToDevice, s));
  FramesOut fo;
  const mv_status st = frames_run(ctx, dev, d_buf, buf_bytes, dev.frm.tab.as<uint64_t>(), dev.frm.tab.as<uint64_t>() + ns,
                                  (uint32_t)ns, s, fo);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);  // (the pageable copies above have been staged; kernels may still run)
    return st;
  }
  sh.n_rows = fo.n_rows;
  sh.n_blk = fo.n_blk;
  sh.rows.resize(8 * fo.n_rows);
  sh.blk_off.resize(fo.n_blk);
  sh.blk_len.resize(fo.n_blk);
  sh.blk_status.resize(fo.n_blk);
  hipError_t e = hipMemcpyAsync(consumed + lo, fo.consumed, 8 * ns, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(drop_msg + lo, fo.drop, 4 * ns, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && fo.n_rows) e = hipMemcpyAsync(sh.rows.data(), fo.rows, 32 * fo.n_rows, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && fo.n_blk) {
    e = hipMemcpyAsync(sh.blk_off.data(), fo.blk_off, 8 * fo.n_blk, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sh.blk_len.data(), fo.blk_len, 8 * fo.n_blk, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sh.blk_status.data(), fo.blk_status, fo.n_blk, hipMemcpyDeviceToHost, s);
  }
  const hipError_t e2 = hipStreamSynchronize(s);
  poll_flags(ctx, dev);
  if (e != hipSuccess || e2 != hipSuccess)
    return set_err(ctx, MV_E_HIP, std::string("mv_verify_frames: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  return MV_OK;
}
}  // namespace

mv_status mv_verify_frames(mv_ctx* ctx, const uint8_t* buf, const uint64_t* soff, const uint64_t* slen, uint32_t ns,
                           uint64_t* consumed, uint32_t* drop_msg, uint32_t* msgs, uint64_t cap_msgs,
                           uint64_t* n_msgs, uint64_t* blk_off, uint64_t* blk_len, uint8_t* blk_status,
                           uint64_t cap_blocks, uint64_t* n_blocks) {
  if (!ctx || !n_msgs || !n_blocks || (ns && (!buf || !soff || !slen || !consumed || !drop_msg)) ||
      (cap_msgs && !msgs) || (cap_blocks && (!blk_off || !blk_len)))
    return set_err(ctx, MV_E_INVALID_ARG, "bad frame args");
  *n_msgs = 0;
  *n_blocks = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  if (ns == 0) return MV_OK;
  // whole streams per device / logical shard, balanced by bytes (mv_shard_plan)
  const size_t nd = ctx->devs.size();
  std::vector<uint64_t> cut;
  if (nd == 1 || ns < 2 * nd) {
    cut = {0, (uint64_t)ns};
  } else {
    std::vector<uint64_t> w(ns);
    for (uint32_t k = 0; k < ns; k++) w[k] = slen[k] + 64;
    cut = balanced_cuts(w.data(), ns, (uint32_t)nd);
  }
  std::vector<FrameShard> shards(cut.size() - 1);
  for (size_t d = 0; d + 1 < cut.size(); d++) {
    shards[d].lo = cut[d];
    shards[d].hi = cut[d + 1];
  }
  mv_status rc;
  if (cut.size() == 2) {
    rc = frames_shard(ctx, ctx->devs[0], buf, soff, slen, consumed, drop_msg, shards[0]);
  } else {
    rc = for_each_cut(ctx, cut, [&](Device& dev, uint64_t lo, uint64_t) -> mv_status {
      size_t d = 0;
      while (shards[d].lo != lo || shards[d].lo == shards[d].hi) d++;
      return frames_shard(ctx, dev, buf, soff, slen, consumed, drop_msg, shards[d]);
    });
  }
  if (rc != MV_OK) return rc;
  // merge: row and block indices rebased to the whole call, offsets to the caller's buffer
  uint64_t rbase = 0, bbase = 0;
  for (FrameShard& sh : shards) {
    if (rbase + sh.n_rows > 0xffffffffull || bbase + sh.n_blk > 0xffffffffull)
      return set_err(ctx, MV_E_INVALID_ARG, "more than 2^32 messages or blocks in one call");
    for (uint64_t r = 0; r < sh.n_rows; r++) {
      uint32_t* row = &sh.rows[8 * r];
      const uint64_t dl = sh.delta[row[0]];
      const uint64_t off = (((uint64_t)row[3] << 32) | row[2]) + dl;
      for (uint64_t k = row[4], e = (uint64_t)row[4] + row[5]; k < e && k < sh.n_blk; k++) {
        if (bbase + k < cap_blocks) {
          blk_off[bbase + k] = sh.blk_off[k] + dl;
          blk_len[bbase + k] = sh.blk_len[k];
          if (blk_status) blk_status[bbase + k] = sh.blk_status[k];
        }
      }
      if (rbase + r < cap_msgs) {
        uint32_t* dst = msgs + 8 * (rbase + r);
        memcpy(dst, row, 32);
        dst[0] = (uint32_t)(sh.lo + row[0]);
        dst[2] = (uint32_t)off;
        dst[3] = (uint32_t)(off >> 32);
        dst[4] = (uint32_t)(bbase + row[4]);
      }
    }
    for (uint64_t k = sh.lo; k < sh.hi; k++)
      if (drop_msg[k] != mv::fr::NONE) drop_msg[k] += (uint32_t)rbase;
    rbase += sh.n_rows;
    bbase += sh.n_blk;
  }
  *n_msgs = rbase;
  *n_blocks = bbase;
  return MV_OK;
}

mv_status mv_dev_verify_frames(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                               const uint64_t* d_soff, const uint64_t* d_slen, uint32_t ns, uint64_t* d_consumed,
                               uint32_t* d_drop_msg, uint32_t* d_msgs, uint64_t cap_msgs, uint64_t* n_msgs,
                               uint64_t* d_blk_off, uint64_t* d_blk_len, uint8_t* d_blk_status, uint64_t cap_blocks,
                               uint64_t* n_blocks, void* stream) {
  if (!ctx || !n_msgs || !n_blocks || (ns && (!d_buf || !d_soff || !d_slen || !d_consumed || !d_drop_msg)) ||
      (cap_msgs && !d_msgs) || (cap_blocks && (!d_blk_off || !d_blk_len)))
    return set_err(ctx, MV_E_INVALID_ARG, "bad frame args");
  if (((uintptr_t)d_buf) & 7) return set_err(ctx, MV_E_INVALID_ARG, "d_buf must be 8-byte aligned");
  *n_msgs = 0;
  *n_blocks = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!committee_ready(ctx)) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  if (ns == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  FramesOut fo;
  const mv_status st = frames_run(ctx, *dev, d_buf, buf_bytes, d_soff, d_slen, ns, s, fo);
  if (st != MV_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  const uint64_t wr = std::min(fo.n_rows, cap_msgs), wb = std::min(fo.n_blk, cap_blocks);
  HIPCHK(ctx, hipMemcpyAsync(d_consumed, fo.consumed, 8 * (size_t)ns, hipMemcpyDeviceToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(d_drop_msg, fo.drop, 4 * (size_t)ns, hipMemcpyDeviceToDevice, s));
  if (wr) HIPCHK(ctx, hipMemcpyAsync(d_msgs, fo.rows, 32 * wr, hipMemcpyDeviceToDevice, s));
  if (wb) {
    HIPCHK(ctx, hipMemcpyAsync(d_blk_off, fo.blk_off, 8 * wb, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_blk_len, fo.blk_len, 8 * wb, hipMemcpyDeviceToDevice, s));
    if (d_blk_status) HIPCHK(ctx, hipMemcpyAsync(d_blk_status, fo.blk_status, wb, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  poll_flags(ctx, *dev);
  *n_msgs = fo.n_rows;
  *n_blocks = fo.n_blk;
  return MV_OK;
}

}  // extern "C"
