// libmysti_verify.so: the block pipeline -- the device passes (enqueue_blocks), the host-parse
// cross-check, the submission queue of mv_verify_blocks and the block entry points.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <utility>

#include "engine_internal.h"

using namespace mvi;

namespace mvi {

// The device block pipeline on stream s (enqueue only): batch-size calls k_block_walk (parse,
// checks and both digests in one pass over the bincode) -> k_block_digest_gate -> batch path
// -> k_block_verdict; smaller calls the committee comb kernels (which parse and hash their own
// blocks on the online path; k_block_ingest -> k_hash_comb_pre -> k_comb_post for small
// batches of long blocks). d_md / d_bd may be null (scratch then).
// own: scratch owned by the caller (a submission-queue pass set, whose reuse is ordered by its
// own completion event): no ring slot, no slot events (two runtime calls less per pass).
mv_status enqueue_blocks(mv_ctx* ctx, Device& dev, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                         const uint64_t* d_len, uint32_t n, uint8_t* d_status, uint8_t* d_md, uint8_t* d_bd,
                         hipStream_t s, DevBuf* own, Device::BlkAux* own_aux) {
  if (n == 0) return MV_OK;
  const mvh::Committee& com = ctx->committee;
  int slot = -1;
  auto& ring = dev.blk.ring;
  // the cross-stream wait is skipped when the slot's previous pass has finished (the common
  // case on the online path, where a wait costs a queue drain)
  if (!own) HIPCHK(ctx, ring.take(s, &slot, /*query_first=*/true));
  DevBuf& scr = own ? *own : ring.slot[slot].scr;
  // small batches of long blocks: the comb verify's signature-only half beside the hash
  // bytes per block from which the split pays (MV_COMB_SPLIT_BYTES: tests and experiments; 0 = never)
  const uint64_t split_bytes = (uint64_t)std::max<int64_t>(0, ctx->kn.comb_split_bytes);
  const bool batch = !(ctx->flags & MV_FLAG_NO_BATCH) && n >= MV_BATCH_MIN;
  const bool split = !batch && !(ctx->flags & MV_FLAG_NO_COMB) && split_bytes && buf_bytes >= split_bytes * (uint64_t)n;
  // scratch: stage | pre_off | pre_len | sig | key_idx | facts | claimed | sig status | md | bd
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t nn = n;
  size_t o = 0;
  const size_t o_stage = o;
  // Batch-size calls (MV_BLK_WALK=1, default): k_block_walk reads each block's bincode once and
  // writes only the per-block outputs, so no P || sig is staged (18.9 GB of HBM
  // traffic less per 2^20 config-4 blocks, and no stage buffer). MV_BLK_WALK=0: the staged form
  // (k_block_ingest stages P || sig, k_b2_lane hashes it); small calls always stage.
  const bool walk = batch && !split && ctx->kn.blk_walk && com.size() <= 512;
  const bool need_stage = !walk;
  o += need_stage ? al(buf_bytes + 256) : al(256);
  const size_t o_poff = o;
  o += al(8 * nn);
  const size_t o_plen = o;
  o += al(8 * nn);
  const size_t o_sig = o;
  o += al(64 * nn);
  const size_t o_kidx = o;
  o += al(4 * nn);
  const size_t o_facts = o;
  o += al(4 * nn);
  const size_t o_claim = o;
  o += al(32 * nn);
  const size_t o_sst = o;
  o += al(nn);
  const size_t o_md = o;
  o += al(32 * nn);
  const size_t o_bd = o;
  o += al(32 * nn);
  const size_t o_q = o;
  if (split) o += 2 * al(144 * nn) + al(nn);
  if (!own && scr.cap < o) {
    // grow every ring slot at once, so the ring never allocates again at this size (the old
    // buffers are retired, not freed: another stream's call may still read them; no drain)
    for (auto& sl : ring.slot) HIPCHK(ctx, sl.scr.ensure(o, sl.done));
  }
  HIPCHK(ctx, scr.ensure(o, own ? nullptr : (hipEvent_t)ring.slot[slot].done));
  char* b = scr.as<char>();
  uint8_t* stage = (uint8_t*)(b + o_stage);
  uint64_t* poff = (uint64_t*)(b + o_poff);
  uint64_t* plen = (uint64_t*)(b + o_plen);
  uint8_t* sig = (uint8_t*)(b + o_sig);
  uint32_t* kidx = (uint32_t*)(b + o_kidx);
  uint32_t* facts = (uint32_t*)(b + o_facts);
  uint8_t* claimed = (uint8_t*)(b + o_claim);
  uint8_t* sst = (uint8_t*)(b + o_sst);
  uint8_t* md = d_md ? d_md : (uint8_t*)(b + o_md);
  uint8_t* bd = d_bd ? d_bd : (uint8_t*)(b + o_bd);
  mvr::EventSet evs;
  mv_status st = make_events(ctx, kBlockStages, evs);
  if (st != MV_OK) return st;
  auto mark = [&](int i) -> hipError_t { return evs.empty() ? hipSuccess : hipEventRecord(evs[i], s); };
  HIPCHK(ctx, mark(0));
  uint8_t* rbuf = (uint8_t*)(b + o_q);
  uint8_t* sbuf = rbuf + al(144 * nn);
  uint8_t* qflags = sbuf + al(144 * nn);
  // short blocks on the online path: the digests are computed inside the committee verify
  // (k_verify_comb16's A wave hashes its blocks before the challenge), one launch less
  // (MV_HASH_IN_COMB=0, A/B: a separate hash launch)
  const bool hash_in_comb = !split && !batch && !(ctx->flags & MV_FLAG_NO_COMB) &&
                            mvk::comb_short_chain(ctx->kn, n) && ctx->kn.hash_in_comb;
  const mvk::BlockHashIn hin{stage, poff, plen, md, bd};
  // ... and the parse too: k_verify_comb16 ingests its own blocks (one wave per block), so an
  // online pass is one kernel launch (MV_INGEST_IN_COMB=0: a separate k_block_ingest, A/B)
  const bool ingest_in_comb = hash_in_comb && ctx->kn.ingest_in_comb;
  const mvk::BlockIngestIn ing{d_buf, d_off, d_len, dev.tab.stakes.as<uint64_t>(), com.size(), com.epoch,
                               com.quorum_threshold, stage, poff, plen, sig, kidx, facts, claimed};
  if (ingest_in_comb) {
    HIPCHK(ctx, mark(1));
  } else if (walk) {
    HIPCHK(ctx, mvk::launch_block_walk(d_buf, d_off, d_len, n, dev.tab.stakes.as<uint64_t>(), com.size(), com.epoch,
                                       com.quorum_threshold, sig, kidx, facts, claimed, md, bd, s));
    HIPCHK(ctx, mark(1));
  } else if (batch && !split && !ctx->stage_timing && n >= 2 * MV_BATCH_MIN + 64 && ctx->kn.blk_pipe && (!own || own_aux)) {
    // Batch-size calls, two halves: the HBM-bound parse of the second half runs on another
    // stream beside the VALU-bound hash of the first (the two streams of a caller's
    // alternating calls otherwise start in phase, parse beside parse). MV_BLK_PIPE=0: one
    // stream. Not under stage timing, whose per-stage events need the stages in sequence.
    // both halves >= MV_BATCH_MIN, so both hash on the batch-size kernel (n >= 2 MV_BATCH_MIN + 64)
    const uint32_t h = ((n / 2) + 63) & ~63u;
    Device::BlkAux& ax = own ? *own_aux : dev.blk.aux[slot];  // (its stream: mv_create)
    for (int k = 0; k < 2; k++) HIPCHK(ctx, ax.ev[k].ensure());
    hipStream_t aux = ax.stream;
    auto parse = [&](uint32_t lo, uint32_t hi, hipStream_t st) {
      return mvk::launch_block_parse(d_buf, d_off + lo, d_len + lo, hi - lo, dev.tab.stakes.as<uint64_t>(), com.size(),
                                     com.epoch, com.quorum_threshold, stage, poff + lo, plen + lo, sig + 64 * (size_t)lo,
                                     kidx + lo, facts + lo, claimed + 32 * (size_t)lo, st);
    };
    auto hash = [&](uint32_t lo, uint32_t hi) {
      return mvk::launch_block_hash(ctx->kn, stage, poff + lo, plen + lo, hi - lo, md + 32 * (size_t)lo,
                                    bd + 32 * (size_t)lo, s);
    };
    HIPCHK(ctx, parse(0, h, s));
    HIPCHK(ctx, hipEventRecord(ax.ev[0], s));
    HIPCHK(ctx, hipStreamWaitEvent(aux, ax.ev[0], 0));
    HIPCHK(ctx, parse(h, n, aux));
    HIPCHK(ctx, hipEventRecord(ax.ev[1], aux));
    HIPCHK(ctx, mark(1));
    HIPCHK(ctx, hash(0, h));
    HIPCHK(ctx, hipStreamWaitEvent(s, ax.ev[1], 0));
    HIPCHK(ctx, hash(h, n));
  } else {
    HIPCHK(ctx, mvk::launch_block_parse(d_buf, d_off, d_len, n, dev.tab.stakes.as<uint64_t>(), com.size(), com.epoch,
                                        com.quorum_threshold, stage, poff, plen, sig, kidx, facts, claimed, s));
    HIPCHK(ctx, mark(1));
    if (split)  // the hash, and beside it on workgroups of their own the signature-only terms
      HIPCHK(ctx, mvk::launch_hash_comb_pre(stage, poff, plen, n, md, bd, sig, dev.tab.combB.p, rbuf, sbuf, qflags, s));
    else if (!hash_in_comb)
      HIPCHK(ctx, mvk::launch_block_hash(ctx->kn, stage, poff, plen, n, md, bd, s));
  }
  // a block whose digest does not match is rejected ahead of its signature (types.rs:327-332):
  // s >= l takes it out of the batch equation, so a tampered block never fails the batch (the
  // per-signature paths need no gate: the verdict puts the digest first)
  if (batch) HIPCHK(ctx, mvk::launch_block_digest_gate(claimed, bd, facts, n, sig, s));
  HIPCHK(ctx, mark(2));
  // the comb kernels write the block verdict themselves (one launch less on the online path);
  // the batch path and the MV_FLAG_NO_COMB ladder leave it to k_block_verdict
  // (MV_VERDICT_FUSED=0, A/B: the separate k_block_verdict)
  const bool fused = ctx->kn.verdict_fused && !batch && !(ctx->flags & MV_FLAG_NO_COMB);
  const mvk::BlockVerdictOut bv{facts, claimed, md, bd, d_status};
  if (batch) {
    st = enqueue_batch(ctx, dev, md, sig, dev.tab.committee_pk.as<uint8_t>(), kidx, n, sst, s, nullptr, nullptr,
                       own == nullptr);  // own == nullptr: mv_dev_verify_blocks on the caller's stream
  } else if (split) {
    HIPCHK(ctx, mvk::launch_comb_post(md, sig, dev.tab.committee_pk.as<uint8_t>(), kidx, n, dev.tab.combA.p,
                                      dev.tab.keyok.as<uint8_t>(), rbuf, sbuf, qflags, sst, s, fused ? &bv : nullptr));
  } else {
    st = enqueue_committee_verify(ctx, dev, md, sig, kidx, n, sst, s, fused ? &bv : nullptr,
                                  hash_in_comb ? &hin : nullptr, ingest_in_comb ? &ing : nullptr);
  }
  if (st != MV_OK) return st;
  HIPCHK(ctx, mark(3));
  if (!fused) HIPCHK(ctx, mvk::launch_block_verdict(facts, claimed, md, bd, sst, n, d_status, s));
  HIPCHK(ctx, mark(4));
  keep_events(ctx, dev.id, kBlockStage0, evs);
  if (!own) HIPCHK(ctx, ring.mark_used(slot, s));
  return MV_OK;
}

// mv_verify_blocks with MV_FLAG_HOST_PARSE: bincode parsed on the host (block_codec.cpp),
// staged pre-images to the device. Kept as the cross-check of the device ingest path.
mv_status verify_blocks_host_parse(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                                   uint32_t n, uint8_t* status, uint8_t* msg_digest, uint8_t* block_digest) {
  const mvh::Committee& com = ctx->committee;
  return for_each_shard(ctx, n, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
    HIPCHK(ctx, hipSetDevice(dev.id));
    uint64_t i = lo;
    std::vector<mvh::BlockFacts> facts;
    while (i < hi) {
      // chunk: <= max_batch blocks and <= 1 GiB of staged pre-images
      uint64_t j = i, bytes = 0;
      while (j < hi && j - i < ctx->max_batch && bytes < (1ull << 30)) bytes += len[j++] + 64 + 16;
      uint32_t m = (uint32_t)(j - i);
      facts.assign(m, mvh::BlockFacts());
      HIPCHK(ctx, dev.hc.h_in.ensure(bytes + 64));
      uint8_t* st = dev.hc.h_in.as<uint8_t>();
      std::vector<uint64_t> soff(m), slen(m);
      std::vector<uint32_t> kidx(m);
      uint64_t pos = 0;
      for (uint32_t k = 0; k < m; k++) {
        mvh::BlockFacts& f = facts[k];
        soff[k] = pos;
        // pre-image is never longer than the bincode (only fields are dropped or re-encoded)
        bool ok = mvh::parse_block(buf + off[i + k], len[i + k], &com, st + pos, len[i + k], f);
        if (!ok) f.parsed = false;
        uint64_t L = ok ? f.preimage_len : 0;
        if (ok) memcpy(st + pos + L, f.signature, 64);
        else memset(st + pos, 0, 64);
        memset(st + pos + L + 64, 0, 8);
        slen[k] = L;
        kidx[k] = (ok && f.author < com.size()) ? (uint32_t)f.author : 0u;
        pos += (L + 64 + 15) & ~7ull;
      }
      HIPCHK(ctx, dev.hc.bytes.ensure(pos + 64));
      HIPCHK(ctx, dev.hc.off.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.len.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.msg.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.out2.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.sig.ensure(64 * (size_t)m));
      HIPCHK(ctx, dev.hc.keyidx.ensure(4 * (size_t)m));
      HIPCHK(ctx, dev.hc.status.ensure(m));
      std::vector<uint8_t> sigs(64 * (size_t)m);
      for (uint32_t k = 0; k < m; k++) {
        const mvh::BlockFacts& f = facts[k];
        memcpy(&sigs[64 * (size_t)k], f.signature, 64);
        // the verdict of a block that fails a check ahead of the signature one does not
        // depend on its signature: s = 2^256 - 1 (>= l) takes it out of the batch
        // equation (rejected up front) instead of failing the whole batch
        if (!f.parsed || f.epoch != com.epoch || f.author >= com.size() || f.round == 0)
          memset(&sigs[64 * (size_t)k + 32], 0xff, 32);
      }
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.bytes.p, st, pos, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.off.p, soff.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.len.p, slen.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.sig.p, sigs.data(), 64 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.keyidx.p, kidx.data(), 4 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      // msg digests stay on the device and feed the verify kernel directly
      HIPCHK(ctx, mvk::launch_block_hash(ctx->kn, dev.hc.bytes.as<uint8_t>(), dev.hc.off.as<uint64_t>(), dev.hc.len.as<uint64_t>(), m,
                                         dev.hc.msg.as<uint8_t>(), dev.hc.out2.as<uint8_t>(), dev.stream));
      if (!(ctx->flags & MV_FLAG_NO_BATCH) && m >= MV_BATCH_MIN) {
        mv_status st2 = enqueue_batch(ctx, dev, dev.hc.msg.as<uint8_t>(), dev.hc.sig.as<uint8_t>(),
                                      dev.tab.committee_pk.as<uint8_t>(), dev.hc.keyidx.as<uint32_t>(), m,
                                      dev.hc.status.as<uint8_t>(), dev.stream, nullptr);
        if (st2 != MV_OK) return st2;
      } else {
        mv_status st2 = enqueue_committee_verify(ctx, dev, dev.hc.msg.as<uint8_t>(), dev.hc.sig.as<uint8_t>(),
                                                 dev.hc.keyidx.as<uint32_t>(), m, dev.hc.status.as<uint8_t>(), dev.stream);
        if (st2 != MV_OK) return st2;
      }
      std::vector<uint8_t> md(32 * (size_t)m), bd(32 * (size_t)m), ss(m);
      HIPCHK(ctx, hipMemcpyAsync(md.data(), dev.hc.msg.p, 32 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(bd.data(), dev.hc.out2.p, 32 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(ss.data(), dev.hc.status.p, m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipStreamSynchronize(dev.stream));
      poll_flags(ctx, dev);
      for (uint32_t k = 0; k < m; k++) {
        status[i + k] = mvh::block_verdict(facts[k], com, &bd[32 * (size_t)k], ss[k]);
        if (!facts[k].parsed) {  // no pre-image: zero digests, as the device path
          memset(&md[32 * (size_t)k], 0, 32);
          memset(&bd[32 * (size_t)k], 0, 32);
        }
        if (msg_digest) memcpy(msg_digest + 32 * (i + k), &md[32 * (size_t)k], 32);
        if (block_digest) memcpy(block_digest + 32 * (i + k), &bd[32 * (size_t)k], 32);
      }
      i = j;
    }
    return MV_OK;
  });
}

// cut[0..parts]: contiguous shards of [0, n) with about equal sums of weights (bytes of
// bincode for block calls): cut[d] is the item boundary whose prefix sum is
// closest to d/parts of the total; every shard is non-empty while n >= parts.
std::vector<uint64_t> balanced_cuts(const uint64_t* w, uint64_t n, uint32_t parts) {
  std::vector<long double> pre(n + 1, 0.0L);
  for (uint64_t i = 0; i < n; i++) pre[i + 1] = pre[i] + (long double)w[i];
  std::vector<uint64_t> cut(parts + 1, n);
  cut[0] = 0;
  for (uint32_t d = 1; d < parts; d++) {
    const long double target = pre[n] * d / parts;
    uint64_t c = (uint64_t)(std::lower_bound(pre.begin(), pre.end(), target) - pre.begin());
    if (c > 0 && c <= n && target - pre[c - 1] < pre[c] - target) c--;
    if (c > n) c = n;
    const uint64_t lo = cut[d - 1] + (n >= parts ? 1 : 0);
    const uint64_t hi = n >= parts ? n - (parts - d) : n;
    cut[d] = c < lo ? lo : (c > hi ? hi : c);
  }
  return cut;
}

// Device passes over lists of blocks gathered from one or several mv_verify_blocks requests.
// A chunk of blocks is packed into a pass set's pinned staging (raw bincode 8-aligned, 16 zero
// bytes after the last block, then the offset and length arrays), read by the GPU (one H2D,
// or zero-copy for small chunks), parsed, hashed and verified there, and its outputs
// [msg digests | block digests | statuses] come back to pinned memory; the verdicts are then
// scattered to each block's owner.
struct BlockItem {
  const uint8_t* p;
  uint64_t len;
  uint8_t *st, *md, *bd;
};

// packed bytes of one block (8-aligned)
inline uint64_t packed_len(const BlockItem& b) { return (b.len + 7) & ~7ull; }

// Chunk limits: <= max_batch blocks and <= MV_BLK_CHUNK_BYTES (default 256 MiB) of bincode.
// A host-fed call larger than one chunk streams: chunk c + 1 is packed, copied and enqueued
// on the other pass set while chunk c runs.
uint64_t chunk_bytes_limit(const mv_ctx* ctx) {
  return ctx->kn.blk_chunk_bytes > 0 ? (uint64_t)ctx->kn.blk_chunk_bytes : (uint64_t)(256ull << 20);
}
uint64_t chunk_end(mv_ctx* ctx, const BlockItem* it, uint64_t lo, uint64_t hi) {
  uint64_t j = lo, bytes = 0;
  const uint64_t lim = chunk_bytes_limit(ctx);
  while (j < hi && j - lo < ctx->max_batch && (bytes < lim || j == lo)) bytes += packed_len(it[j++]);
  return j;
}

// Copies items [lo, hi) into h (their packed offsets in off[], lengths in len[]), on up to
// `threads` threads for large chunks.
void pack_items(uint8_t* h, uint64_t* off, uint64_t* len, const BlockItem* it, uint64_t lo, uint64_t hi,
                size_t buf_bytes, int64_t pack_threads) {
  const uint32_t m = (uint32_t)(hi - lo);
  uint64_t pos = 0;
  for (uint32_t k = 0; k < m; k++) {
    off[k] = pos;
    len[k] = it[lo + k].len;
    pos += packed_len(it[lo + k]);
  }
  auto copy = [&](uint32_t a, uint32_t b) {
    for (uint32_t k = a; k < b; k++) {
      const uint64_t l = len[k], o = off[k];
      memcpy(h + o, it[lo + k].p, l);
      memset(h + o + l, 0, ((l + 7) & ~7ull) - l);
    }
  };
  // MV_PACK_THREADS: host threads packing a large chunk (0: min(8, cores))
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned max_thr = pack_threads > 0 ? (unsigned)pack_threads : std::min(8u, hw ? hw : 4u);
  const unsigned threads = pos < (8u << 20) ? 1u : std::min<unsigned>(max_thr, m);
  if (threads <= 1) {
    copy(0, m);
  } else {  // item ranges of about equal bytes
    std::vector<std::thread> th;
    uint32_t a = 0;
    for (unsigned t = 1; t <= threads; t++) {
      const uint64_t target = pos * t / threads;
      uint32_t b = a;
      while (b < m && off[b] < target) b++;
      if (t == threads) b = m;
      if (b > a) {
        if (t == threads) copy(a, b);
        else th.emplace_back(copy, a, b);
      }
      a = b;
    }
    for (auto& x : th) x.join();
  }
  memset(h + pos, 0, buf_bytes - pos);
}

mv_status ensure_pass_set(mv_ctx* ctx, Device& dev, int s) {
  // (ps.stream is qstream[s], a stream of its own made by mv_create: not the host-buffer
  // signature path's copy / compute streams)
  HIPCHK(ctx, dev.pass.set[s].done.ensure());
  return MV_OK;
}

// Packs items [lo, hi) into pass set s of dev and enqueues the device pipeline on its stream
// (no wait). The set must be idle. A large chunk whose blocks already lie in page-locked
// caller memory (mv_host_alloc), in order with small gaps, skips the host pack: the DMA engine
// reads the caller's bytes in place (only the offset / length arrays are staged), so the
// host's memory bandwidth is not spent on a second copy.
mv_status enqueue_block_chunk(mv_ctx* ctx, Device& dev, int s, const BlockItem* it, uint64_t lo, uint64_t hi) {
  HIPCHK(ctx, hipSetDevice(dev.id));
  mv_status rc = ensure_pass_set(ctx, dev, s);
  if (rc != MV_OK) return rc;
  Device::PassSet& ps = dev.pass.set[s];
  const bool trace = ctx->kn.blk_trace != 0;  // diagnostics (MV_BLK_TRACE): host-side times
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = trace ? now() : 0;
  const uint32_t m = (uint32_t)(hi - lo);
  uint64_t bytes = 0;
  for (uint64_t k = lo; k < hi; k++) bytes += packed_len(it[k]);
  // small chunks (the online path): the ingest kernel reads the pinned staging over PCIe
  // itself (zero-copy) instead of waiting for an H2D copy and the launch behind it
  const uint64_t zc_max = (uint64_t)std::max<int64_t>(0, ctx->kn.blk_zerocopy);  // MV_BLK_ZEROCOPY=<bytes> (0: always copy)
  // in-place DMA of pinned caller bytes (see above)
  const uint8_t* base = it[lo].p;
  uint64_t span = 0;
  bool direct = bytes > zc_max && host_pinned(base);
  for (uint64_t k = lo; k < hi && direct; k++) {
    if (it[k].p < base || (uint64_t)(it[k].p - base) < span) direct = false;  // in order, no overlap
    span = (uint64_t)(it[k].p - base) + it[k].len;
  }
  // any alignment (the ingest kernels read from the aligned word at or below a block's start);
  // gaps between blocks are copied too, so they must stay small
  // ... and [base, base + span) must lie inside ONE page-locked allocation: a pass merges
  // several callers' items, and two callers' buffers may sit close together with unpinned (or
  // unmapped) memory between them
  direct = direct && span && span <= 2 * bytes + 4096 && pinned_range_holds(base, span);
  const size_t buf_bytes = direct ? (span + 16 + 15) & ~(size_t)15 : (bytes + 16 + 15) & ~(size_t)15;
  const size_t o_off = buf_bytes, o_len = o_off + 8 * (size_t)m, total = o_len + 8 * (size_t)m;
  HIPCHK(ctx, ps.h_in.ensure(direct ? 16 * (size_t)m : total));
  uint8_t* h = ps.h_in.as<uint8_t>();
  if (direct) {
    uint64_t* hoff = reinterpret_cast<uint64_t*>(h);
    uint64_t* hlen = hoff + m;
    for (uint32_t k = 0; k < m; k++) {
      hoff[k] = (uint64_t)(it[lo + k].p - base);
      hlen[k] = it[lo + k].len;
    }
  } else {
    pack_items(h, (uint64_t*)(h + o_off), (uint64_t*)(h + o_len), it, lo, hi, buf_bytes, ctx->kn.pack_threads);
  }
  HIPCHK(ctx, ps.bytes.ensure(total));
  HIPCHK(ctx, ps.out2.ensure(65 * (size_t)m + 256));
  HIPCHK(ctx, ps.h_out.ensure(65 * (size_t)m));
  const double t1 = trace ? now() : 0;
  const uint8_t* dbuf = nullptr;
  uint8_t* hout_dev = nullptr;  // zero-copy outputs too: the kernels write the pinned h_out
  if (direct) {
    uint8_t* d = ps.bytes.as<uint8_t>();
    HIPCHK(ctx, hipMemcpyAsync(d, base, span, hipMemcpyHostToDevice, ps.stream));
    HIPCHK(ctx, hipMemsetAsync(d + span, 0, buf_bytes - span, ps.stream));  // the 16 readable bytes past the end
    HIPCHK(ctx, hipMemcpyAsync(d + o_off, h, 16 * (size_t)m, hipMemcpyHostToDevice, ps.stream));
    dbuf = d;
  } else if (total <= zc_max) {
    void* dp = nullptr;
    void* dq = nullptr;
    // outputs only under the comb path: the batch path re-reads the digests many times
    const bool zc_out = m < MV_BATCH_MIN;
    if (hipHostGetDevicePointer(&dp, h, 0) == hipSuccess && dp &&
        (!zc_out || (hipHostGetDevicePointer(&dq, ps.h_out.p, 0) == hipSuccess && dq))) {
      dbuf = static_cast<const uint8_t*>(dp);
      hout_dev = static_cast<uint8_t*>(dq);
    } else {
      (void)hipGetLastError();
    }
  }
  if (!dbuf) {
    HIPCHK(ctx, hipMemcpyAsync(ps.bytes.p, h, total, hipMemcpyHostToDevice, ps.stream));
    dbuf = ps.bytes.as<uint8_t>();
  }
  const double t2 = trace ? now() : 0;
  uint8_t* dout = hout_dev ? hout_dev : ps.out2.as<uint8_t>();
  rc = enqueue_blocks(ctx, dev, dbuf, buf_bytes, (const uint64_t*)(dbuf + o_off), (const uint64_t*)(dbuf + o_len), m,
                      dout + 64 * (size_t)m, dout, dout + 32 * (size_t)m, ps.stream, &ps.scr, &ps.aux);
  if (rc != MV_OK) {
    (void)hipStreamSynchronize(ps.stream);  // what was queued reads the staging
    return rc;
  }
  // from here on an error must drain the stream first: the queued kernels read the staging
  hipError_t e = hout_dev ? hipSuccess : hipMemcpyAsync(ps.h_out.p, dout, 65 * (size_t)m, hipMemcpyDeviceToHost, ps.stream);
  if (e == hipSuccess) e = hipEventRecord(ps.done, ps.stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ps.stream);
    return set_err(ctx, MV_E_HIP, std::string("block pass: ") + hipGetErrorString(e));
  }
  ps.it = it;
  ps.lo = lo;
  ps.m = m;
  ps.inflight = true;
  if (trace)
    fprintf(stderr, "[blk] set %d, %u blocks%s: pack %.1f, h2d %.1f, kernels %.1f us\n", s, m, direct ? " (in place)" : "",
            t1 - t0, t2 - t1, now() - t2);
  return MV_OK;
}

// Waits for pass set s's chunk and scatters its verdicts and digests to the blocks' owners.
// Needs no context lock (the set is owned by the caller until it is marked idle).
mv_status finish_block_chunk(mv_ctx* ctx, Device& dev, int s) {
  Device::PassSet& ps = dev.pass.set[s];
  if (!ps.inflight) return MV_OK;
  ps.inflight = false;
  HIPCHK(ctx, hipSetDevice(dev.id));
  // MV_PASS_SPIN=1 (A/B): the pass owner polls its event instead of blocking in the runtime
  const bool spin = ctx->kn.pass_spin != 0;
  hipError_t e;
  if (spin) {
    while ((e = hipEventQuery(ps.done)) == hipErrorNotReady) std::this_thread::yield();
  } else {
    e = hipEventSynchronize(ps.done);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ps.stream);
    return set_err(ctx, MV_E_HIP, std::string("block pass: ") + hipGetErrorString(e));
  }
  const BlockItem* it = static_cast<const BlockItem*>(ps.it);
  const uint32_t m = ps.m;
  const uint8_t* ho = ps.h_out.as<uint8_t>();
  for (uint32_t k = 0; k < m; k++) {
    const BlockItem& b = it[ps.lo + k];
    *b.st = ho[64 * (size_t)m + k];
    if (b.md) memcpy(b.md, ho + 32 * (size_t)k, 32);
    if (b.bd) memcpy(b.bd, ho + 32 * ((size_t)m + k), 32);
  }
  return MV_OK;
}

// Items [lo, hi) on dev in chunks over both pass sets (chunk c + 1 packed and enqueued while
// chunk c runs); returns when all are scattered. Caller holds ctx->mu and owns both sets.
mv_status verify_block_items(mv_ctx* ctx, Device& dev, const BlockItem* it, uint64_t lo, uint64_t hi) {
  mv_status rc = MV_OK;
  int s = 0;
  for (uint64_t i = lo; i < hi && rc == MV_OK; s ^= 1) {
    rc = finish_block_chunk(ctx, dev, s);  // the set's chunk before last
    if (rc != MV_OK) break;
    const uint64_t j = chunk_end(ctx, it, i, hi);
    rc = enqueue_block_chunk(ctx, dev, s, it, i, j);
    i = j;
  }
  for (int k = 0; k < 2; k++) {
    const mv_status r2 = finish_block_chunk(ctx, dev, k);
    if (rc == MV_OK) rc = r2;
  }
  poll_flags(ctx, dev);
  return rc;
}

// One pass of the submission queue over the requests the combining caller took. set >= 0:
// the pass fits one chunk per device and runs on that pass set: it is packed and enqueued
// under ctx->mu, `enqueued()` is called, and the caller waits for the device without the
// lock (the next pass can be packed meanwhile). set < 0: a large pass that owns both sets
// and streams its chunks (`enqueued()` at the end). Every request gets rc (and err).
template <class Enqueued>
void run_block_requests(mv_ctx* ctx, std::deque<mv_ctx::BlockReq*>& reqs, int set, Enqueued enqueued) {
  bool signalled = false;
  auto signal = [&] {
    if (!signalled) {
      signalled = true;
      enqueued();
    }
  };
  std::string err;
  mv_status rc = MV_OK;
  std::vector<BlockItem> items;
  std::vector<std::pair<size_t, std::pair<uint64_t, uint64_t>>> shards;  // device, [lo, hi)
  try {
    size_t total = 0;
    for (auto* r : reqs) total += r->n;
    items.reserve(total);
    for (auto* r : reqs)
      for (uint32_t k = 0; k < r->n; k++)
        items.push_back(BlockItem{r->buf + r->off[k], r->len[k], r->status + k,
                                  r->md ? r->md + 32 * (size_t)k : nullptr, r->bd ? r->bd + 32 * (size_t)k : nullptr});
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->q_passes++;
    t_err = &err;
    const size_t nd = ctx->devs.size();
    std::vector<uint64_t> cut;
    if (nd == 1 || items.size() < 2 * nd) {
      cut = {0, (uint64_t)items.size()};
    } else {
      std::vector<uint64_t> w(items.size());
      for (size_t k = 0; k < items.size(); k++) w[k] = items[k].len + 64;  // bytes, plus a per-block constant
      cut = balanced_cuts(w.data(), w.size(), (uint32_t)nd);
    }
    // the committee is checked again under the lock: a failed mv_set_committee may have
    // unpublished it after the request was queued
    if (!committee_ready(ctx)) {
      rc = set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
    } else if (set >= 0) {
      shards.reserve(cut.size());  // push_back below must not throw once a chunk is in flight
      for (size_t d = 0; d + 1 < cut.size() && rc == MV_OK; d++) {
        if (cut[d] == cut[d + 1]) continue;
        rc = enqueue_block_chunk(ctx, ctx->devs[d], set, items.data(), cut[d], cut[d + 1]);
        if (rc == MV_OK) shards.push_back({d, {cut[d], cut[d + 1]}});
      }
    } else if (cut.size() == 2) {
      rc = verify_block_items(ctx, ctx->devs[0], items.data(), 0, items.size());
    } else {
      rc = for_each_cut(ctx, cut, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
        return verify_block_items(ctx, dev, items.data(), lo, hi);
      });
      if (rc != MV_OK) err = ctx->err;
    }
    t_err = nullptr;
  } catch (...) {  // std::bad_alloc from the item list or the shard plan
    t_err = nullptr;
    rc = MV_E_ALLOC;
    err = "mv_verify_blocks: host allocation failed";
  }
  signal();
  // set >= 0: wait for this pass's chunks (outside the context lock) and scatter the verdicts
  for (auto& sh : shards) {
    t_err = &err;
    const mv_status r2 = finish_block_chunk(ctx, ctx->devs[sh.first], set);
    t_err = nullptr;
    if (rc == MV_OK) rc = r2;
  }
  if (set >= 0 && !shards.empty()) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto& sh : shards) poll_flags(ctx, ctx->devs[sh.first]);
  }
  for (auto* r : reqs) {
    r->rc = rc;
    if (rc != MV_OK) r->err = err;
  }
}

}  // namespace mvi

extern "C" {

mv_status mv_verify_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                           uint8_t* status, uint8_t* msg_digest, uint8_t* block_digest) {
  if (!ctx || (n && (!buf || !off || !len || !status))) return set_err(ctx, MV_E_INVALID_ARG, "bad block args");
  if (!ctx->has_committee) {
    // a committee change in progress holds com_mu: wait for it rather than fail the call
    std::shared_lock<std::shared_mutex> cl(ctx->com_mu);
    if (!ctx->has_committee) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  }
  if (n == 0) return MV_OK;
  if (ctx->flags & MV_FLAG_HOST_PARSE) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return verify_blocks_host_parse(ctx, buf, off, len, n, status, msg_digest, block_digest);
  }
  // the resident online service: small calls, no queue, no launch
  {
    uint64_t bytes = 0, longest = 0;
    for (uint32_t k = 0; k < n && bytes <= (128u << 10); k++) {
      bytes += (len[k] + 7) & ~7ull;
      longest = std::max<uint64_t>(longest, len[k]);
    }
    if (online_eligible(ctx, n, bytes, longest)) {
      std::shared_lock<std::shared_mutex> cl(ctx->com_mu);
      if (committee_ready(ctx)) {
        // one service per physical GPU: logical shards of one device (shards_per_device) share
        // the first shard's, so there is one resident kernel per GPU, not one per shard
        Device& dev = ctx->devs[ctx->online_devs[ctx->online_rr.fetch_add(1) % ctx->online_devs.size()]];
        {
          std::lock_guard<std::mutex> lk(ctx->mu);  // the service object (devs is fixed after mv_create)
          if (!dev.online) dev.online = std::make_shared<OnlineSvc>();
        }
        if (dev.online->failed) goto queue_path;  // a failed service: the submission queue serves
        std::string err;
        t_err = &err;
        const mv_status rc = online_verify(ctx, dev, buf, off, len, n, status, msg_digest, block_digest);
        t_err = nullptr;
        if (rc != MV_OK) {
          std::lock_guard<std::mutex> lk(ctx->mu);
          ctx->err = err;
        }
        return rc;
      }
    }
  }
queue_path:
  // Flat combining, pipelined: the request joins the queue; a caller that finds no pass being
  // packed and a free pass set takes every queued request (its own included) into one pass,
  // packs and enqueues it, then lets the next caller pack the following pass into the other
  // set while its own runs on the device. n - 1 peer tasks each submitting a block or two
  // (net_sync.rs:214-221, 314-386) thus share GPU round trips, up to q_sets passes in flight.
  mv_ctx::BlockReq req{buf, off, len, n, status, msg_digest, block_digest};
  ctx->q_calls++;
  const int linger_us = (int)ctx->kn.q_linger_us;  // MV_Q_LINGER_US, default 50 (profiles/r03/ab/queue_linger_*)
  // MV_Q_SPIN_US: a caller whose request is in another caller's pass polls for its verdicts
  // that long before sleeping on the queue's condition variable (no wake-up convoy on q_mu)
  const int spin_us = (int)ctx->kn.q_spin_us;
  bool lingered = false, spun = false;
  std::unique_lock<std::mutex> ql(ctx->q_mu);
  ctx->q.push_back(&req);
  if (ctx->q_lingering) ctx->q_linger_cv.notify_one();
  auto any_busy = [ctx] {
    for (int k = 0; k < ctx->q_sets; k++)
      if (ctx->q_set_busy[k]) return true;
    return false;
  };
  auto mark_all = [ctx](bool v) {
    for (int k = 0; k < ctx->q_sets; k++) ctx->q_set_busy[k] = v;
  };
  while (!req.done) {
    int s = -1;
    for (int k = 0; k < ctx->q_sets && s < 0; k++)
      if (!ctx->q_set_busy[k]) s = k;
    if (req.taken && spin_us > 0 && !spun) {
      spun = true;
      ql.unlock();
      const auto dl = std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us);
      while (!req.done.load(std::memory_order_acquire) && std::chrono::steady_clock::now() < dl)
        std::this_thread::yield();
      ql.lock();
      continue;
    }
    if (ctx->q_packing || ctx->q_lingering || s < 0 || ctx->q.empty()) {
      ctx->q_cv.wait(ql);
      continue;
    }
    // Callers released together by a pass come back within microseconds of each other; the
    // first one back waits (bounded) for the others instead of starting a pass of one, so the
    // passes stay as large as the callers' groups (a lone caller's last pass carried 1: no wait)
    if (linger_us > 0 && !lingered && ctx->q.size() < ctx->q_last_calls) {
      lingered = true;
      ctx->q_lingering = true;
      const auto dl = std::chrono::steady_clock::now() + std::chrono::microseconds(linger_us);
      while (ctx->q.size() < ctx->q_last_calls && ctx->q_linger_cv.wait_until(ql, dl) != std::cv_status::timeout) {
      }
      ctx->q_lingering = false;
      ctx->q_cv.notify_all();
      continue;
    }
    std::deque<mv_ctx::BlockReq*> batch;
    batch.swap(ctx->q);  // no allocation
    for (auto* r : batch) r->taken = true;
    uint64_t blocks = 0, bytes = 0;
    for (auto* r : batch) {
      blocks += r->n;
      for (uint32_t k = 0; k < r->n; k++) bytes += (r->len[k] + 7) & ~7ull;
    }
    // larger than one chunk per device: the pass streams its chunks over both sets
    const uint64_t nd = ctx->devs.size();
    const bool big = blocks > (uint64_t)ctx->max_batch * nd || bytes > chunk_bytes_limit(ctx) * nd;
    ctx->q_packing = true;
    if (big)
      while (any_busy()) ctx->q_cv.wait(ql);
    const int set = big ? -1 : s;
    if (big) mark_all(true);
    else ctx->q_set_busy[s] = true;
    ql.unlock();
    run_block_requests(ctx, batch, set, [ctx] {
      std::lock_guard<std::mutex> lk(ctx->q_mu);
      ctx->q_packing = false;
      ctx->q_cv.notify_all();
    });
    ql.lock();
    ctx->q_last_calls = batch.size();
    for (auto* r : batch) r->done = true;
    if (big) mark_all(false);
    else ctx->q_set_busy[s] = false;
    ctx->q_cv.notify_all();
  }
  ql.unlock();
  if (req.rc != MV_OK) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->err = req.err;
  }
  return req.rc;
}

mv_status mv_shard_plan(const uint64_t* weights, uint64_t n, uint32_t parts, uint64_t* cut) {
  if ((n && !weights) || !cut || parts == 0) return MV_E_INVALID_ARG;
  std::vector<uint64_t> c = balanced_cuts(weights, n, parts);
  memcpy(cut, c.data(), sizeof(uint64_t) * (parts + 1));
  return MV_OK;
}

mv_status mv_dev_verify_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                               const uint64_t* d_off, const uint64_t* d_len, uint32_t n, uint8_t* d_status,
                               uint8_t* d_msg_digest, uint8_t* d_block_digest, void* stream) {
  if (!ctx || (n && (!d_buf || !d_off || !d_len || !d_status))) return set_err(ctx, MV_E_INVALID_ARG, "bad args");
  if (((uintptr_t)d_buf) & 7) return set_err(ctx, MV_E_INVALID_ARG, "d_buf must be 8-byte aligned");
  if ((((uintptr_t)d_msg_digest) | ((uintptr_t)d_block_digest)) & 15)
    return set_err(ctx, MV_E_INVALID_ARG, "digest arrays must be 16-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->has_committee) return set_err(ctx, MV_E_NO_COMMITTEE, "mv_set_committee first");
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  return enqueue_blocks(ctx, *dev, d_buf, buf_bytes, d_off, d_len, n, d_status, d_msg_digest, d_block_digest, s);
}

int64_t mv_frame_blocks(const uint8_t* buf, uint64_t len, uint64_t* off, uint64_t* blen, uint64_t cap,
                        uint64_t* consumed) {
  constexpr uint64_t kMaxSize = 16ull << 20;  // Network::MAX_SIZE (network.rs:216)
  constexpr uint64_t kPingRest = 8;           // PING_SIZE 12 - the size word (network.rs:425, 563)
  auto le = [&](uint64_t p, int bytes) {
    uint64_t v = 0;
    for (int k = 0; k < bytes; k++) v |= (uint64_t)buf[p + k] << (8 * k);
    return v;
  };
  if (consumed) *consumed = 0;
  if (len && !buf) return -1;
  if (cap && (!off || !blen)) return -1;
  uint64_t p = 0, found = 0;
  while (len - p >= 4) {
    const uint64_t size = ((uint64_t)buf[p] << 24) | ((uint64_t)buf[p + 1] << 16) | ((uint64_t)buf[p + 2] << 8) | buf[p + 3];
    if (size > kMaxSize) return -1;
    const uint64_t body = p + 4, need = size ? size : kPingRest;
    if (len - body < need) break;  // an incomplete frame: wait for more bytes
    const uint64_t end = body + need;
    if (size) {
      if (size < 4) return -1;  // no room for the message tag
      const uint64_t tag = le(body, 4);
      if (tag > 4) return -1;
      if (tag == 1 || tag == 3) {  // Blocks / RequestBlocksResponse: Vec<Data<StatementBlock>>
        if (end - body < 12) return -1;
        const uint64_t count = le(body + 4, 8);
        uint64_t q = body + 12;
        for (uint64_t k = 0; k < count; k++) {
          if (end - q < 8) return -1;
          const uint64_t l = le(q, 8);
          q += 8;
          if (l > end - q) return -1;
          if (found < cap) {
            off[found] = q;
            blen[found] = l;
          }
          found++;
          q += l;
        }
      }
    }
    p = end;
    if (consumed) *consumed = p;
  }
  return (int64_t)found;
}

}  // extern "C"
