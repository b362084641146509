// libmysti_verify.so: contexts, device sharding and the C ABI of include/mysti_verify.h.
//
// One mv_ctx owns, per HIP device: a stream; the fixed-base tables ([0..128]B and
// [0..128](2^124 B) for the ladders, the comb table C_B); the committee (keys, stakes, the
// per-key comb tables C_A); growable device / pinned-host buffers. Host-buffer calls split
// their items into one contiguous shard per device and run each shard on its own host
// thread (one stream per device, no collective: only per-item verdicts come back), in
// chunks of at most cfg.max_batch items. Calls on one ctx are serialised by a mutex.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dirent.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"

using namespace mvi;

namespace mvi {

constexpr int kGuardBatches = 64;  // batches cut into sub-batch equations after a failure
// Dense failures (config 3: ~1% of the signatures bad, so every sub-batch equation fails and the
// whole batch is re-verified after a wasted MSM): a guarded batch that failed in at least half
// of its groups sends the next kSingleRun batches straight to the single path. Each of those
// counts its rejected signatures; while a batch holds at least kDenseRejects of them the run is
// renewed, otherwise the equation is tried again (guarded). The run is longer than the batches a
// caller can have in flight (kFlagRing): a renewal is seen only when a single-path batch
// completes, and a run that ran out before then sent a batch back to a doomed equation (config
// 3 with three streams: 2 of 10 batches). Recovery does not wait for the run: the first clean
// single-path batch to complete ends it.
constexpr int kSingleRun = 32;
constexpr uint32_t kDenseRejects = 4;
constexpr uint32_t kSingleMark = 0x80000000u;  // flag_groups entry of a single-path batch

// Buffers that grow retire the old allocation instead of freeing it at once: hipFree /
// hipHostFree drain the whole device, which would wait for the resident online kernel (it lives
// while online traffic flows) and for every other stream's calls. A retired block may still be
// read by work in flight: `guard` (when set) is the completion event of the ring slot it served,
// recorded after every call that used the slot, so its completion means no call still reads it
// (a later record on the same slot completes later still); blocks without a guard served only
// synchronous host-buffer calls, which had finished when they were retired. reap_ready frees
// what is safe whenever the device's online service is not running (the drain is then bounded
// by the calls in flight), and growth is geometric (x1.5), so a sequence of growing calls
// retires O(log n) blocks, not one per call. reap_retired (mv_destroy,
// mv_set_committee: the service stopped) frees the rest.
struct Retired {
  int device;
  void* p;
  bool host;
  hipEvent_t guard;
};
std::mutex g_retired_mu;
std::vector<Retired> g_retired;
std::atomic<int> g_retired_n{0};

void free_retired(const std::vector<Retired>& blocks) {
  for (const Retired& r : blocks) (void)(r.host ? hipHostFree(r.p) : hipFree(r.p));
  mvr::g_live -= (int64_t)blocks.size();
}

// Frees the retired blocks of `device` (its current device must be set; drains the device).
void reap_retired(int device) {
  std::vector<Retired> mine;
  {
    std::lock_guard<std::mutex> lk(g_retired_mu);
    auto it = std::stable_partition(g_retired.begin(), g_retired.end(),
                                    [device](const Retired& r) { return r.device != device; });
    mine.assign(it, g_retired.end());
    g_retired.erase(it, g_retired.end());
    g_retired_n.store((int)g_retired.size());
  }
  free_retired(mine);
}

// Frees the retired blocks of `device` that no call in flight can read (guard complete or
// none); the caller has checked that no resident kernel runs on the device.
void reap_ready(int device) {
  if (g_retired_n.load(std::memory_order_relaxed) == 0) return;
  std::vector<Retired> done;
  {
    std::lock_guard<std::mutex> lk(g_retired_mu);
    auto it = std::stable_partition(g_retired.begin(), g_retired.end(), [device](const Retired& r) {
      if (r.device != device) return true;
      if (!r.guard) return false;
      const hipError_t q = hipEventQuery(r.guard);
      if (q != hipSuccess) (void)hipGetLastError();  // hipErrorNotReady: still in use
      return q != hipSuccess;
    });
    done.assign(it, g_retired.end());
    g_retired.erase(it, g_retired.end());
    g_retired_n.store((int)g_retired.size());
  }
  free_retired(done);
}

}  // namespace mvi

void mvr::retire(void* p, bool host, hipEvent_t guard) {
  int d = 0;
  (void)hipGetDevice(&d);
  std::lock_guard<std::mutex> lk(g_retired_mu);
  g_retired.push_back(Retired{d, p, host, guard});
  g_retired_n.store((int)g_retired.size());
  g_live++;
}

namespace mvi {

// Accounts the batch flags of every slot whose last call has completed (non-blocking):
// counters, and the adaptive group policy (a failed equation arms the guard).
void poll_flags(mv_ctx* ctx, Device& dev) {
  for (int k = 0; k < Device::kFlagRing; k++) {
    const uint32_t ng = dev.batch.flag_groups[k];
    if (!ng) continue;
    if (hipEventQuery(dev.batch.flag_ev[k]) != hipSuccess) {
      (void)hipGetLastError();  // hipErrorNotReady: still running
      continue;
    }
    dev.batch.flag_groups[k] = 0;
    const uint32_t* f = dev.batch.flags(k);
    if (ng == kSingleMark) {  // a single-path batch: f[0] = its rejected signatures
      if (f[0] >= kDenseRejects) {
        ctx->single_left.store(kSingleRun);
      } else {
        ctx->single_left.store(0);
        ctx->guard_left = kGuardBatches;  // back to the equation, guarded
      }
      continue;
    }
    ctx->batches++;
    ctx->groups_run += ng;
    uint32_t bad = 0;
    for (uint32_t g = 0; g < ng; g++) bad += f[1 + g] ? 0u : 1u;
    ctx->groups_failed += bad;
    if (!f[0]) {
      ctx->fallbacks++;
      ctx->guard_left = kGuardBatches;
      if (ng >= 2 && 2 * bad >= ng && ctx->groups_fixed == 0) {  // dense: the MSM was wasted
        ctx->dense_failures++;
        ctx->single_left.store(kSingleRun);
      }
    }
  }
}

uint32_t pick_groups(mv_ctx* ctx) {
  if (ctx->groups_fixed) return ctx->groups_fixed;
  if (ctx->guard_left.fetch_sub(1) > 0) return ctx->guard_groups;
  ctx->guard_left.store(0);
  return ctx->base_groups;
}

// Enqueues the batch path (batch.hip) for n signatures on stream s. flag_dst (optional,
// device) receives the all-groups flag word.
mv_status enqueue_batch(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk,
                        const uint32_t* d_key_idx, uint32_t n, uint8_t* d_status, hipStream_t s,
                        uint32_t* flag_dst, const mvk::ChunkGate* gate, bool caller_stream) {
  poll_flags(ctx, dev);
  // the scratch slot is claimed here and waited for below, once the route is known: the single
  // route uses no batch scratch and must not make s wait for the slot's last user
  auto& ring = dev.batch.ring;
  int slot;
  HIPCHK(ctx, ring.claim(&slot));
  if (!dev.batch.h_flags.p) {
    constexpr size_t kFlagBytes = sizeof(uint32_t) * Device::kFlagRing * Device::kFlagWords;
    HIPCHK(ctx, dev.batch.h_flags.ensure(kFlagBytes));
    memset(dev.batch.h_flags.p, 0, kFlagBytes);
  }
  const int fe = dev.batch.flag_next;
  dev.batch.flag_next = (fe + 1) % Device::kFlagRing;
  HIPCHK(ctx, dev.batch.flag_ev[fe].ensure());
  if (dev.batch.flag_groups[fe]) {  // kFlagRing calls in flight: the oldest must be accounted before its words are reused
    HIPCHK(ctx, hipEventSynchronize(dev.batch.flag_ev[fe]));
    poll_flags(ctx, dev);
  }
  const bool com_a = d_key_idx && dev.committee_loaded && d_pk == dev.tab.committee_pk.as<uint8_t>() &&
                     !(ctx->flags & MV_FLAG_NO_COMB);
  if (ctx->groups_fixed == 0 && ctx->single_left.load() > 0) {
    // dense failures (kSingleRun): every signature verified alone, no combined equation; the
    // rejected count decides whether the next batches try the equation again (poll_flags)
    ctx->single_left--;
    ring.hand_back(slot);  // no batch scratch used
    if (gate && gate->n)
      for (uint32_t c = 0; c < gate->n; c++) HIPCHK(ctx, hipStreamWaitEvent(s, gate->ready[c], 0));
    mv_status st = com_a ? enqueue_committee_verify(ctx, dev, d_msg, d_sig, d_key_idx, n, d_status, s)
                         : enqueue_verify(ctx, dev, d_msg, d_sig, d_pk, d_key_idx, n, d_status, s);
    if (st != MV_OK) return st;
    HIPCHK(ctx, dev.batch.rejects.ensure(sizeof(uint32_t) * Device::kFlagRing));
    uint32_t* cnt = dev.batch.rejects.as<uint32_t>() + fe;
    HIPCHK(ctx, mvk::launch_count_rejects(d_status, n, cnt, s));
    if (flag_dst) HIPCHK(ctx, hipMemsetAsync(flag_dst, 0, 4, s));  // no combination was checked
    HIPCHK(ctx, hipMemcpyAsync(dev.batch.flags(fe), cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipEventRecord(dev.batch.flag_ev[fe], s));
    dev.batch.flag_groups[fe] = kSingleMark;
    ctx->single_batches++;
    return MV_OK;
  }
  HIPCHK(ctx, ring.order_behind(slot, s));
  auto& sl = ring.slot[slot];
  const uint32_t groups = pick_groups(ctx);
  // scratch for the largest group count, so the adaptive policy never reallocates
  HIPCHK(ctx, sl.scr.b.ensure(mvk::batch_scratch_bytes(n, mvk::BATCH_MAX_GROUPS), sl.done));
  HIPCHK(ctx, sl.scr.v.ensure(mvk::verify_scratch_bytes(n), sl.done));
  uint32_t key[10];
  memcpy(key, ctx->secret, 32);
  const uint64_t call = ctx->calls.fetch_add(1);
  key[8] = (uint32_t)call;
  key[9] = (uint32_t)(call >> 32);
  uint32_t* flag = nullptr;
  mvr::EventSet evs;
  mv_status st = make_events(ctx, mvk::BATCH_STAGES, evs);
  if (st != MV_OK) return st;
  // committee keys (com_a): A comes from the comb tables built at mv_set_committee (no
  // per-signature decode)
  hipEvent_t chain[2] = {};
  // on a caller's stream only when asked (MV_PREP_CHAIN=2): the chain orders the caller's streams
  // behind each other's preparations, which the caller may not expect (its own gates could then
  // deadlock them)
  const bool chained = ctx->kn.prep_chain && !(gate && gate->n) && (!caller_stream || ctx->kn.prep_chain >= 2);
  if (chained) {
    HIPCHK(ctx, dev.batch.prep_chain.ensure());
    chain[0] = dev.batch.prep_chained ? (hipEvent_t)dev.batch.prep_chain : nullptr;
    chain[1] = dev.batch.prep_chain;
  }
  HIPCHK(ctx, mvk::launch_verify_batch(ctx->kn, d_msg, d_sig, d_pk, d_key_idx, n, groups, key, dev.tab.btab.p, sl.scr.b.p,
                                       sl.scr.v.p, d_status, s, &flag, evs.empty() ? nullptr : evs.data(),
                                       com_a ? dev.tab.combA.p : nullptr, com_a ? dev.tab.keyok.as<uint8_t>() : nullptr,
                                       com_a ? (uint32_t)ctx->committee.size() : 0u, dev.tab.combB.p, gate,
                                       chained ? chain : nullptr));
  if (chained) dev.batch.prep_chained = true;
  keep_events(ctx, dev.id, 0, evs);
  if (flag_dst) HIPCHK(ctx, hipMemcpyAsync(flag_dst, flag, 4, hipMemcpyDeviceToDevice, s));
  const uint32_t ng = (n + mvk::batch_group_size(n, groups) - 1) / mvk::batch_group_size(n, groups);
  HIPCHK(ctx, hipMemcpyAsync(dev.batch.flags(fe), flag, sizeof(uint32_t) * (1 + ng), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, ring.mark_used(slot, s));
  HIPCHK(ctx, hipEventRecord(dev.batch.flag_ev[fe], s));
  dev.batch.flag_groups[fe] = ng;
  return MV_OK;
}

// k_verify (single path) on stream s with the device's scratch ring (per-wave tables)
mv_status enqueue_verify(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk,
                         const uint32_t* d_key_idx, uint32_t n, uint8_t* d_status, hipStream_t s) {
  if (n == 0) return MV_OK;
  auto& ring = dev.single.ring;
  int slot;
  HIPCHK(ctx, ring.take(s, &slot));
  auto& sl = ring.slot[slot];
  // (growth retires the old buffer, which another stream's call may still read: no drain)
  HIPCHK(ctx, sl.scr.ensure(mvk::verify_scratch_bytes(n), sl.done));
  HIPCHK(ctx, mvk::launch_verify(d_msg, d_sig, d_pk, d_key_idx, n, dev.tab.btab.p, sl.scr.p, d_status, s));
  HIPCHK(ctx, ring.mark_used(slot, s));
  return MV_OK;
}

// Committee-key signatures one by one: comb tables (comb.hip) or, with MV_FLAG_NO_COMB,
// the per-signature ladder (k_verify).
// bv: the block verdict fused into the comb kernel (the block path); null otherwise.
mv_status enqueue_committee_verify(mv_ctx* ctx, Device& dev, const uint8_t* d_msg, const uint8_t* d_sig,
                                   const uint32_t* d_kidx, uint32_t n, uint8_t* d_status, hipStream_t s,
                                   const mvk::BlockVerdictOut* bv, const mvk::BlockHashIn* hin,
                                   const mvk::BlockIngestIn* ing) {
  if (!(ctx->flags & MV_FLAG_NO_COMB)) {
    HIPCHK(ctx, mvk::launch_verify_comb(ctx->kn, d_msg, d_sig, dev.tab.committee_pk.as<uint8_t>(), d_kidx, n, dev.tab.combB.p,
                                        dev.tab.combA.p, dev.tab.keyok.as<uint8_t>(), d_status, s, bv, hin, ing));
  } else {
    return enqueue_verify(ctx, dev, d_msg, d_sig, dev.tab.committee_pk.as<uint8_t>(), d_kidx, n, d_status, s);
  }
  return MV_OK;
}

bool committee_ready(mv_ctx* ctx) {
  if (!ctx->has_committee) return false;
  for (auto& dev : ctx->devs)
    if (!dev.committee_loaded) return false;
  return true;
}

// True if p is page-locked host memory the DMA engines can read directly (mv_host_alloc,
// hipHostMalloc, hipHostRegister, torch pin_memory).
bool host_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: the query fails; do not leave the error set
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// True if [p, p + bytes) lies inside the one page-locked host allocation that holds p (the
// allocation's address range from the runtime). False when the runtime cannot say.
bool pinned_range_holds(const void* p, uint64_t bytes) {
  if (!host_pinned(p)) return false;
  void* start = nullptr;
  size_t size = 0;
  hipDeviceptr_t q = const_cast<void*>(p);
  if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, q) != hipSuccess ||
      hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, q) != hipSuccess || !start || !size) {
    (void)hipGetLastError();
    return false;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(start), b = reinterpret_cast<uintptr_t>(p);
  return b >= a && b - a <= size && bytes <= size - (b - a);
}

// mv_ed25519_verify's batch path over [lo, hi) of pinned caller arrays, in a few large
// batches (two by default) on two compute streams. The DMA engines copy a batch's inputs
// chunk by chunk on a copy stream, and k_bv_prep of chunk c starts as soon as chunk c has
// landed, so the PCIe copy overlaps the preparation; batch t + 1's copy and preparation run
// beside batch t's sort, buckets and tail (two input buffers, reuse ordered by events).
// Enqueue only (ctx->mu held): the statuses land in dev.pin.sig_stage[slot], complete once both of
// dev.pin.sig_done[slot] have; the caller waits for them without the lock (mv_ed25519_verify).
mv_status verify_host_streamed(mv_ctx* ctx, Device& dev, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk,
                               const uint32_t* key_idx, uint64_t lo, uint64_t hi, int slot) {
  const int chunk_log2 = (int)std::min<int64_t>(24, std::max<int64_t>(8, ctx->kn.stream_chunk_log2));  // MV_STREAM_CHUNK_LOG2
  const uint64_t m = hi - lo;
  // Batch sizes: shares of the call (MV_STREAM_FRACS, separated by ',' or '/'; default 0.7,0.3). The
  // last batch's prep, sort, buckets and tail follow the last copy, so the shares decrease;
  // every batch is whole 1,024s, >= MV_BATCH_MIN and <= max_batch (more batches when needed).
  // (A streaming MSM -- one batch whose chunks are sorted and bucketed during the copy window --
  // measured slower, 181-198 against 208 M/s, and was removed in round 6: DESIGN.md 13.)
  const std::vector<double> fracs(ctx->kn.stream_fracs, ctx->kn.stream_fracs + ctx->kn.n_stream_fracs);
  std::vector<uint32_t> sizes;
  {
    double tot = 0.0;
    for (double f : fracs) tot += f;
    uint64_t done = 0;
    for (size_t k = 0; k < fracs.size() && done < m; k++) {
      uint64_t want = k + 1 == fracs.size() ? m - done : (((uint64_t)(m * fracs[k] / tot)) + 1023) & ~1023ull;
      if (want < MV_BATCH_MIN) want = MV_BATCH_MIN;
      if (want > m - done) want = m - done;
      if (m - done - want > 0 && m - done - want < MV_BATCH_MIN) want = m - done;  // no runt batch
      if (want > ctx->max_batch) want = ctx->max_batch;
      done += want;
      sizes.push_back((uint32_t)want);
    }
    while (done < m) {  // larger than the shares allow (max_batch): whole max_batch batches
      const uint64_t want = std::min<uint64_t>(m - done, ctx->max_batch);
      sizes.push_back((uint32_t)want);
      done += want;
    }
  }
  uint32_t cap = 0;
  for (uint32_t z : sizes) cap = std::max(cap, z);
  uint32_t chunk = 1u << chunk_log2;
  while ((cap + chunk - 1) / chunk > (uint32_t)Device::kMaxChunks / 2) chunk <<= 1;
  // chunk schedule of a batch of k: the first batch starts with small chunks (2^14, 2^15, ...
  // signatures), so the chip starts preparing after ~40 us of copying instead of a whole chunk's
  auto schedule = [&](int first, uint32_t k) {
    std::vector<uint32_t> cut;
    uint32_t o = 0, c = first ? std::min<uint32_t>(chunk, 1u << 14) : chunk;
    while (o < k) {
      cut.push_back(o);
      o += c;
      if (c < chunk) c *= 2;
    }
    cut.push_back(k);
    return cut;
  };
  const size_t kb = pk ? 32 : 4;  // pk rows or committee key indices
  for (int b = 0; b < Device::kPinBufs; b++) {
    HIPCHK(ctx, dev.pin.pin_free[b].ensure());
    HIPCHK(ctx, dev.pin.chunk_ev[b].ensure(Device::kMaxChunks, hipEventDisableTiming));
    // (a buffer grown while another call's batch still reads it is retired behind pin_free[b])
    HIPCHK(ctx, dev.pin.pin_msg[b].ensure(32 * (size_t)cap, dev.pin.pin_free[b]));
    HIPCHK(ctx, dev.pin.pin_sig[b].ensure(64 * (size_t)cap, dev.pin.pin_free[b]));
    HIPCHK(ctx, dev.pin.pin_pk[b].ensure(kb * cap, dev.pin.pin_free[b]));
    HIPCHK(ctx, dev.pin.pin_st[b].ensure(cap, dev.pin.pin_free[b]));
  }
  for (int k = 0; k < 2; k++) HIPCHK(ctx, dev.pin.sig_done[slot][k].ensure());
  HIPCHK(ctx, dev.pin.sig_stage[slot].ensure(m));
  uint8_t* hst = dev.pin.sig_stage[slot].as<uint8_t>();
  bool used[2] = {false, false};
  // copies on the device stream (host-buffer signature calls are serialised by ctx->mu, and the
  // block passes have streams of their own); batch t computes on pstream[t & 1]. mv_create makes
  // these three streams first, so they sit on three distinct hardware queues (GPU_MAX_HW_QUEUES
  // = 4; later streams share queues round-robin, and a copy queued behind another stream's
  // kernels would serialise the pipeline)
  hipStream_t xs = dev.stream;
  uint64_t i = lo;
  for (size_t t = 0; t < sizes.size(); i += sizes[t], t++) {
    // input buffers and compute streams rotate across calls too, so a second caller's first batch
    // copies into a buffer the first caller's batches are not using
    const int rot = dev.pin.pin_next++;
    const int b = rot % Device::kPinBufs, ci = rot & 1;
    hipStream_t cs = dev.pin.pstream[ci];
    used[ci] = true;
    const uint32_t k = sizes[t];
    // buffer b is free once the last batch that used it (this call's or another's) is done
    HIPCHK(ctx, hipStreamWaitEvent(xs, dev.pin.pin_free[b], 0));
    const uint8_t* src_pk = pk ? pk + 32 * i : (const uint8_t*)(key_idx + i);
    const std::vector<uint32_t> cut = schedule(t == 0, k);
    std::vector<uint32_t> marks;  // chunk ends, signatures
    for (uint32_t c = 0; c + 1 < cut.size() && cut[c] < k; c++) {
      const uint32_t o = cut[c];
      const size_t r = std::min(cut[c + 1], k) - o;
      marks.push_back(o + (uint32_t)r);
      HIPCHK(ctx, hipMemcpyAsync(dev.pin.pin_msg[b].as<uint8_t>() + 32 * (size_t)o, msg + 32 * (i + o), 32 * r,
                                 hipMemcpyHostToDevice, xs));
      HIPCHK(ctx, hipMemcpyAsync(dev.pin.pin_sig[b].as<uint8_t>() + 64 * (size_t)o, sig + 64 * (i + o), 64 * r,
                                 hipMemcpyHostToDevice, xs));
      HIPCHK(ctx, hipMemcpyAsync(dev.pin.pin_pk[b].as<uint8_t>() + kb * o, src_pk + kb * o, kb * r,
                                 hipMemcpyHostToDevice, xs));
      HIPCHK(ctx, hipEventRecord(dev.pin.chunk_ev[b][c], xs));
    }
    // every chunk's prep on cs (a second prep stream per compute stream measured slower:
    // 163-167 vs 175-180 M/s; more streams than the 4 hardware queues share queues)
    const mvk::ChunkGate gate{dev.pin.chunk_ev[b].data(), (uint32_t)marks.size(), marks.data()};
    mv_status rc = enqueue_batch(ctx, dev, dev.pin.pin_msg[b].as<uint8_t>(), dev.pin.pin_sig[b].as<uint8_t>(),
                                 pk ? dev.pin.pin_pk[b].as<uint8_t>() : dev.tab.committee_pk.as<uint8_t>(),
                                 pk ? nullptr : dev.pin.pin_pk[b].as<uint32_t>(), k, dev.pin.pin_st[b].as<uint8_t>(), cs,
                                 nullptr, &gate);
    hipError_t e = rc == MV_OK ? hipMemcpyAsync(hst + (i - lo), dev.pin.pin_st[b].p, k, hipMemcpyDeviceToHost, cs)
                               : hipSuccess;
    if (e == hipSuccess && rc == MV_OK) e = hipEventRecord(dev.pin.pin_free[b], cs);
    if (rc != MV_OK || e != hipSuccess) {
      // drain what was queued (it reads the input buffers and writes h_out) before returning
      (void)hipStreamSynchronize(xs);
      (void)hipStreamSynchronize(dev.pin.pstream[0]);
      (void)hipStreamSynchronize(dev.pin.pstream[1]);
      if (rc != MV_OK) return rc;
      return set_err(ctx, MV_E_HIP, std::string("streamed verify: ") + hipGetErrorString(e));
    }
  }
  for (int k = 0; k < 2; k++) HIPCHK(ctx, hipEventRecord(dev.pin.sig_done[slot][k], dev.pin.pstream[used[k] ? k : 1 - k]));
  return MV_OK;
}

}  // namespace mvi

// ---- runtime switches (mvk::Knobs) -------------------------------------------
// Read from the environment once, at mv_create -- as the reference reads its knobs at start-up
// (validator.rs:104-119, config.rs:39-100) -- never per call: a multi-threaded host may call
// setenv, and getenv racing it is undefined behaviour. mv_set_option changes one afterwards.
namespace {
enum KnobKind { K_ON, K_OFF, K_FLAG, K_INT };  // on unless "0..." | on iff "1..." | on if set | integer
struct KnobDef {
  const char* name;
  int64_t mvk::Knobs::*field;
  KnobKind kind;
  bool create_only;  // consumed by mv_create: mv_set_option refuses it
};
const KnobDef kKnobs[] = {
    {"MV_BLK_PIPE", &mvk::Knobs::blk_pipe, K_ON, false},
    {"MV_COMB_SPLIT_BYTES", &mvk::Knobs::comb_split_bytes, K_INT, false},
    {"MV_HASH_IN_COMB", &mvk::Knobs::hash_in_comb, K_ON, false},
    {"MV_INGEST_IN_COMB", &mvk::Knobs::ingest_in_comb, K_ON, false},
    {"MV_VERDICT_FUSED", &mvk::Knobs::verdict_fused, K_ON, false},
    {"MV_BLK_CHUNK_BYTES", &mvk::Knobs::blk_chunk_bytes, K_INT, false},
    {"MV_PACK_THREADS", &mvk::Knobs::pack_threads, K_INT, false},
    {"MV_BLK_TRACE", &mvk::Knobs::blk_trace, K_FLAG, false},
    {"MV_BLK_ZEROCOPY", &mvk::Knobs::blk_zerocopy, K_INT, false},
    {"MV_PASS_SPIN", &mvk::Knobs::pass_spin, K_OFF, false},
    {"MV_PASS_SETS", &mvk::Knobs::pass_sets, K_INT, true},
    {"MV_Q_LINGER_US", &mvk::Knobs::q_linger_us, K_INT, false},
    {"MV_Q_SPIN_US", &mvk::Knobs::q_spin_us, K_INT, false},
    {"MV_ONLINE", &mvk::Knobs::online, K_ON, false},
    {"MV_ONLINE_LONG", &mvk::Knobs::online_long, K_ON, false},
    {"MV_ONLINE_PRIO", &mvk::Knobs::online_prio, K_ON, false},
    {"MV_ONLINE_WGS", &mvk::Knobs::online_wgs, K_INT, false},
    {"MV_ONLINE_IDLE_US", &mvk::Knobs::online_idle_us, K_INT, false},
    {"MV_ONLINE_TRACE", &mvk::Knobs::online_trace, K_FLAG, false},
    {"MV_ONLINE_DEBUG", &mvk::Knobs::online_debug, K_FLAG, false},
    {"MV_ONLINE_INJECT", &mvk::Knobs::online_inject, K_OFF, false},
    {"MV_ONLINE_SPINNERS", &mvk::Knobs::online_spinners, K_INT, false},
    {"MV_STREAM_CHUNK_LOG2", &mvk::Knobs::stream_chunk_log2, K_INT, false},
    {"MV_GUARD_GROUPS", &mvk::Knobs::guard_groups, K_INT, true},
    {"MV_BASE_GROUPS", &mvk::Knobs::base_groups, K_INT, true},
    {"MV_NO_KEY_AGG", &mvk::Knobs::no_key_agg, K_OFF, false},
    {"MV_REDUCE_QUAD", &mvk::Knobs::reduce_quad, K_INT, false},
    {"MV_B2_LANE", &mvk::Knobs::b2_lane, K_ON, false},
    {"MV_COMB_QUAD", &mvk::Knobs::comb_quad, K_INT, false},
    {"MV_PREP_CHAIN", &mvk::Knobs::prep_chain, K_INT, false},
    {"MV_BLK_WALK", &mvk::Knobs::blk_walk, K_ON, false},
    {"MV_BUCKET_BAL", &mvk::Knobs::bucket_bal, K_INT, false},
    {"MV_SORT_WIDE", &mvk::Knobs::sort_wide, K_OFF, false},
    {"MV_FINAL_ROWS", &mvk::Knobs::final_rows, K_ON, false},
    {"MV_REDUCE_ROWS", &mvk::Knobs::reduce_rows, K_INT, false},
    {"MV_INDEX_TAG_BITS", &mvk::Knobs::index_tag_bits, K_INT, false},
};

// read-only (mv_get_option): the process-wide count of live device resources (dev_resources.h)
const char kLiveResources[] = "MV_LIVE_RESOURCES";

const KnobDef* find_knob(const char* name) {
  if (!name) return nullptr;
  for (const KnobDef& d : kKnobs)
    if (strcmp(d.name, name) == 0) return &d;
  return nullptr;
}

mvk::Knobs knobs_from_env() {
  mvk::Knobs k;
  for (const KnobDef& d : kKnobs) {
    const char* e = getenv(d.name);
    if (!e || (!*e && d.kind != K_FLAG)) continue;
    switch (d.kind) {
      case K_ON: k.*d.field = e[0] != '0'; break;
      case K_OFF: k.*d.field = e[0] == '1'; break;
      case K_FLAG: k.*d.field = 1; break;
      case K_INT: k.*d.field = atoll(e); break;
    }
  }
  if (const char* e = getenv("MV_STREAM_FRACS")) {  // shares separated by ',' or '/'
    int n = 0;
    std::string x = e;
    for (size_t q = 0; q < x.size() && n < 8;) {
      size_t c = x.find_first_of(",/", q);
      if (c == std::string::npos) c = x.size();
      const double f = atof(x.substr(q, c - q).c_str());
      if (f > 0.0) k.stream_fracs[n++] = f;
      q = c + 1;
    }
    if (n == 0) k.stream_fracs[n++] = 1.0;
    k.n_stream_fracs = n;
  }
  return k;
}
}  // namespace

extern "C" {

const char* mv_version(void) { return "mysti_verify 0.2 gfx950"; }

}  // extern "C"

namespace mvi {

// Frees the retired buffers of `dev` that no call in flight reads (reap_ready), unless the
// online service of its GPU is running (its kernel would hold the free's device drain). Called
// with ctx->mu held at the start of the calls that grow buffers; o.mu is held across the check
// and the frees, so no launch starts in between.
void reap_idle(mv_ctx* ctx, Device& dev) {
  if (g_retired_n.load(std::memory_order_relaxed) == 0) return;
  std::shared_ptr<OnlineSvc> o;
  for (Device& d : ctx->devs)
    if (d.id == dev.id && d.online) o = d.online;  // one service per GPU (the first logical shard's)
  if (!o) {
    reap_ready(dev.id);
    return;
  }
  std::lock_guard<std::mutex> lk(o->mu);
  if (o->stuck) return;
  if (o->launched) {
    const hipError_t q = hipEventQuery(o->res.exited);
    if (q != hipSuccess) {
      (void)hipGetLastError();  // running (hipErrorNotReady)
      return;
    }
  }
  reap_ready(dev.id);
}

}  // namespace mvi

extern "C" {

mv_status mv_host_alloc(mv_ctx* ctx, uint64_t bytes, void** out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad host_alloc args");
  *out = nullptr;
  if (bytes == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(ctx->devs[0].id));
  if (hipHostMalloc(out, bytes, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return set_err(ctx, MV_E_ALLOC, "hipHostMalloc failed");
  }
  return MV_OK;
}

void mv_host_free(mv_ctx* ctx, void* p) {
  (void)ctx;
  if (p) (void)hipHostFree(p);
}

int64_t mv_block_preimage(const uint8_t* bincode, uint64_t len, uint8_t* out, uint64_t cap) {
  if (!bincode && len) return -1;
  mvh::BlockFacts f;
  if (!mvh::parse_block(bincode, len, nullptr, out, out ? cap : 0, f)) return -1;
  return (int64_t)f.preimage_len;
}


mv_status mv_set_option(mv_ctx* ctx, const char* name, int64_t value) {
  if (!ctx) return MV_E_INVALID_ARG;
  if (name && strcmp(name, kLiveResources) == 0) return set_err(ctx, MV_E_INVALID_ARG, std::string(name) + " is read-only");
  const KnobDef* d = find_knob(name);
  if (!d) return set_err(ctx, MV_E_INVALID_ARG, std::string("unknown option ") + (name ? name : "(null)"));
  if (d->create_only) return set_err(ctx, MV_E_INVALID_ARG, std::string(name) + " is read at mv_create only");
  if (d->field == &mvk::Knobs::index_tag_bits && (value < 1 || value > 64))
    return set_err(ctx, MV_E_INVALID_ARG, std::string(name) + " takes 1..64");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->kn.*d->field = d->kind == K_INT ? value : (value != 0);
  return MV_OK;
}

mv_status mv_get_option(mv_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !value) return MV_E_INVALID_ARG;
  if (name && strcmp(name, kLiveResources) == 0) {
    *value = mvr::g_live.load();
    return MV_OK;
  }
  const KnobDef* d = find_knob(name);
  if (!d) return set_err(ctx, MV_E_INVALID_ARG, std::string("unknown option ") + (name ? name : "(null)"));
  *value = ctx->kn.*d->field;
  return MV_OK;
}

mv_status mv_create(const mv_config* cfg, mv_ctx** out) {
  if (!out) return MV_E_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MV_E_NO_DEVICE;
  uint32_t mask = cfg && cfg->device_mask ? cfg->device_mask : 1u;
  mv_ctx* ctx = new mv_ctx();
  if (cfg && cfg->max_batch) ctx->max_batch = cfg->max_batch;
  if (cfg) ctx->flags = cfg->flags;
  ctx->kn = knobs_from_env();  // the only environment read: every switch, once
  if (ctx->kn.guard_groups >= 1 && ctx->kn.guard_groups <= mvk::BATCH_MAX_GROUPS)  // sub-batches while guarded
    ctx->guard_groups = (uint32_t)ctx->kn.guard_groups;
  if (ctx->kn.base_groups >= 1 && ctx->kn.base_groups <= mvk::BATCH_MAX_GROUPS)  // sub-batches when not guarded
    ctx->base_groups = (uint32_t)ctx->kn.base_groups;
  // two passes in flight: four measured worse on 16 concurrent 1-block callers (68.0 k vs
  // 72.2 k blocks/s, p99 203 vs 146 us; profiles/r03/c5_pass_sets.txt)
  ctx->q_sets = 2;
  if (ctx->kn.pass_sets >= 2 && ctx->kn.pass_sets <= Device::kPassSets) ctx->q_sets = (int)ctx->kn.pass_sets;
  {
    FILE* f = fopen("/dev/urandom", "rb");
    size_t got = f ? fread(ctx->secret, 1, sizeof(ctx->secret), f) : 0;
    if (got == sizeof(ctx->secret) && fread(ctx->index_secret, 1, sizeof(ctx->index_secret), f) != sizeof(ctx->index_secret))
      got = 0;
    if (f) fclose(f);
    if (got != sizeof(ctx->secret)) {
      delete ctx;
      return MV_E_INVALID_ARG;  // no entropy source: refuse rather than use predictable z_i
    }
  }
  // shards_per_device > 1: several logical devices (stream + buffers each) per HIP device;
  // host-buffer calls shard across them as across GPUs (tests the sharding on one GPU)
  const uint32_t reps = cfg && cfg->shards_per_device > 1 ? (cfg->shards_per_device > 8 ? 8 : cfg->shards_per_device) : 1;
  for (int d = 0; d < 32; d++) {
    if (!(mask & (1u << d))) continue;
    if (d >= ndev) {
      delete ctx;
      return MV_E_NO_DEVICE;
    }
    for (uint32_t r = 0; r < reps; r++) {
      ctx->devs.emplace_back();
      ctx->devs.back().id = d;
    }
  }
  for (auto& dev : ctx->devs) {
    hipError_t e = hipSetDevice(dev.id);
    if (e == hipSuccess) e = dev.stream.create();
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = dev.pin.pstream[k].create();
    // every other stream the engine uses, now: the runtime spreads streams over its hardware
    // queues (GPU_MAX_HW_QUEUES) in creation order, and the online service's stream must be
    // created after all of them, or a stream made later can share its queue and wait behind the
    // resident kernel (test_online_service_does_not_block_other_streams)
    for (int k = 0; k < Device::kPassSets && e == hipSuccess; k++) {
      e = dev.pass.qstream[k].create();
      dev.pass.set[k].stream = dev.pass.qstream[k];
    }
    for (int k = 0; k < Device::kPassSets && e == hipSuccess; k++) e = dev.pass.set[k].aux.stream.create();
    for (int k = 0; k < Device::kBlkSlots && e == hipSuccess; k++) e = dev.blk.aux[k].stream.create();
    if (e == hipSuccess) e = dev.tab.btab.ensure(mvk::btable_bytes());
    if (e == hipSuccess) e = mvk::launch_btable_init(dev.tab.btab.p, dev.stream);
    if (e == hipSuccess) e = dev.tab.combB.ensure(mvk::comb_table_bytes(1));
    if (e == hipSuccess) e = mvk::launch_comb_init(nullptr, 1, 0, dev.tab.combB.p, nullptr, dev.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev.stream);
    if (e != hipSuccess) {
      mv_destroy(ctx);
      return MV_E_HIP;
    }
  }
  for (size_t i = 0; i < ctx->devs.size(); i++)
    if (i == 0 || ctx->devs[i].id != ctx->devs[i - 1].id) ctx->online_devs.push_back(i);
  *out = ctx;
  return MV_OK;
}

// Names the step a teardown is in on stderr while it takes longer than 5 s (a stall in
// mv_destroy otherwise looks like a silent hang to whoever waits for the process).
class PhaseWatch {
 public:
  explicit PhaseWatch(const char* what) : what_(what), th_([this] { run(); }) {}
  ~PhaseWatch() {
    {
      std::lock_guard<std::mutex> lk(m_);
      done_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void phase(const char* p) { phase_.store(p); }

 private:
  void run() {
    std::unique_lock<std::mutex> lk(m_);
    for (int s = 5; !cv_.wait_for(lk, std::chrono::seconds(5), [this] { return done_; }); s += 5) {
      fprintf(stderr, "[%s] still in '%s' after %d s\n", what_, phase_.load(), s);
      if (s == 5) dump_threads();
    }
  }
  // every thread's name, kernel wait channel and current system call (/proc/self/task): tells a
  // runtime wait on a GPU signal (ioctl) from one on a lock (futex)
  static void dump_threads() {
    DIR* d = opendir("/proc/self/task");
    if (!d) return;
    while (dirent* e = readdir(d)) {
      if (e->d_name[0] == '.') continue;
      char path[128], comm[64] = {0}, wchan[64] = {0}, sc[160] = {0};
      auto rd = [&](const char* f, char* out, size_t cap) {
        snprintf(path, sizeof path, "/proc/self/task/%s/%s", e->d_name, f);
        if (FILE* fp = fopen(path, "r")) {
          size_t k = fread(out, 1, cap - 1, fp);
          out[k] = 0;
          fclose(fp);
          for (char* c = out; *c; c++)
            if (*c == '\n') *c = ' ';
        }
      };
      rd("comm", comm, sizeof comm);
      rd("wchan", wchan, sizeof wchan);
      rd("syscall", sc, sizeof sc);
      fprintf(stderr, "  tid %s %s wchan=%s syscall=%s\n", e->d_name, comm, wchan, sc);
    }
    closedir(d);
  }
  const char* what_;
  std::atomic<const char*> phase_{"start"};
  std::mutex m_;
  std::condition_variable cv_;
  bool done_ = false;
  std::thread th_;
};

void mv_destroy(mv_ctx* ctx) {
  if (!ctx) return;
  PhaseWatch watch("mv_destroy");
  watch.phase("stage events");
  (void)mv_stage_times(ctx, nullptr, nullptr, 1);  // drain pending stage events
  bool stuck = false;
  {
    watch.phase("online service stop");
    std::unique_lock<std::shared_mutex> cl(ctx->com_mu);
    for (auto& dev : ctx->devs)
      if (dev.online) {
        std::lock_guard<std::mutex> ol(dev.online->mu);
        (void)hipSetDevice(dev.id);
        online_release(*dev.online);  // before the device drain below: the kernel would hold it
        stuck |= dev.online->stuck;
      }
  }
  if (stuck) {
    // a resident launch that would not end still reads the engine's buffers: freeing them (or a
    // device drain, which would wait for it) is unsafe, so the context is abandoned, not freed
    fprintf(stderr, "[mv_destroy] the online service did not stop: the context's device memory is leaked\n");
    return;
  }
  for (auto& dev : ctx->devs) {
    (void)hipSetDevice(dev.id);
    watch.phase("engine stream drain");
    if (dev.stream) (void)hipStreamSynchronize(dev.stream);
    watch.phase("device drain");
    (void)hipDeviceSynchronize();  // device-API calls may have run on the caller's streams
    watch.phase("retired buffers");
    reap_retired(dev.id);
    // one release per group, members in declaration order (the device is idle: no order matters)
    watch.phase("frees: tables, host-call, WAL, frame and index buffers");
    mvr::reset(dev.tab);
    mvr::reset(dev.hc);
    mvr::reset(dev.wal);
    mvr::reset(dev.frm);
    mvr::reset(dev.index);
    mvr::reset(dev.seal);
    mvr::reset(dev.encode);
    mvr::reset(dev.votes);
    watch.phase("frees: batch and single path");
    mvr::reset(dev.batch);
    mvr::reset(dev.single);
    watch.phase("frees: block ring, aux streams");
    mvr::reset(dev.blk);
    watch.phase("frees: pinned signature path, copy streams");
    mvr::reset(dev.pin);
    watch.phase("frees: pass sets, queue streams");
    mvr::reset(dev.pass);
    watch.phase("frees: engine stream");
    dev.stream.release();
  }
  watch.phase("context");
  delete ctx;
}

const char* mv_last_error(const mv_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

mv_status mv_set_committee(mv_ctx* ctx, const uint8_t* pks, const uint64_t* stakes, uint32_t n, uint64_t epoch,
                           uint8_t* key_ok) {
  if (!ctx || !pks || !stakes || n == 0 || n > 512) return set_err(ctx, MV_E_INVALID_ARG, "bad committee args");
  // total = checked sum (committee.rs:50-54: "Total stake overflow"); 2 * total must fit as well,
  // or the quorum threshold 2 * total / 3 would wrap and almost any parent set would pass it
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++)
    if (__builtin_add_overflow(total, stakes[i], &total))
      return set_err(ctx, MV_E_INVALID_ARG, "committee stakes: the total stake does not fit in 64 bits");
  if (total > UINT64_MAX / 2)
    return set_err(ctx, MV_E_INVALID_ARG, "committee stakes: twice the total stake does not fit in 64 bits");
  std::unique_lock<std::shared_mutex> cl(ctx->com_mu);  // no online request in flight
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (auto& dev : ctx->devs)
    if (dev.online) {
      std::lock_guard<std::mutex> ol(dev.online->mu);
      (void)hipSetDevice(dev.id);
      if (!online_stop(*dev.online))  // the resident kernel reads the tables rebuilt below
        return set_err(ctx, MV_E_HIP, "online service: the resident kernel did not stop");
    }
  mvh::Committee c;
  c.pks.assign(pks, pks + 32 * (size_t)n);
  c.stakes.assign(stakes, stakes + n);
  c.epoch = epoch;
  c.quorum_threshold = 2 * total / 3;
  // unpublish first: if a device step fails below, the context is left with no committee
  // (block calls then refuse with MV_E_NO_COMMITTEE) rather than host facts that disagree
  // with half-built device tables
  ctx->has_committee = false;
  for (auto& dev : ctx->devs) dev.committee_loaded = false;
  for (auto& dev : ctx->devs) {
    HIPCHK(ctx, hipSetDevice(dev.id));
    HIPCHK(ctx, hipDeviceSynchronize());  // earlier device-API work may still read the old tables
    reap_retired(dev.id);                 // (the service is stopped: the drain waits for no resident kernel)
    HIPCHK(ctx, dev.tab.committee_pk.ensure(32 * (size_t)n));
    HIPCHK(ctx, dev.tab.stakes.ensure(8 * (size_t)n));
    HIPCHK(ctx, dev.tab.combA.ensure(mvk::comb_table_bytes(n)));
    HIPCHK(ctx, dev.tab.keyok.ensure(n));
    HIPCHK(ctx, hipMemcpyAsync(dev.tab.committee_pk.p, pks, 32 * (size_t)n, hipMemcpyHostToDevice, dev.stream));
    HIPCHK(ctx, hipMemcpyAsync(dev.tab.stakes.p, stakes, 8 * (size_t)n, hipMemcpyHostToDevice, dev.stream));
    // VerificationKey::try_from once per key (ZIP-215 decode) and its comb table of -A
    HIPCHK(ctx, mvk::launch_comb_init(dev.tab.committee_pk.as<uint8_t>(), n, 1, dev.tab.combA.p, dev.tab.keyok.as<uint8_t>(),
                                      dev.stream));
    HIPCHK(ctx, hipStreamSynchronize(dev.stream));
  }
  if (key_ok) {
    Device& dev = ctx->devs[0];
    HIPCHK(ctx, hipSetDevice(dev.id));
    HIPCHK(ctx, hipMemcpy(key_ok, dev.tab.keyok.p, n, hipMemcpyDeviceToHost));
  }
  ctx->committee = std::move(c);
  for (auto& dev : ctx->devs) dev.committee_loaded = true;
  ctx->has_committee = true;
  return MV_OK;
}

mv_status mv_blake2b256(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                        uint8_t* out) {
  if (!ctx || (n && (!buf || !off || !len || !out))) return set_err(ctx, MV_E_INVALID_ARG, "bad blake2b args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  return for_each_shard(ctx, n, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
    HIPCHK(ctx, hipSetDevice(dev.id));
    uint64_t i = lo;
    while (i < hi) {
      // chunk by count and by staged bytes (<= 1 GiB)
      uint64_t j = i, bytes = 0;
      while (j < hi && j - i < ctx->max_batch && bytes < (1ull << 30)) bytes += (len[j++] + 15) & ~7ull;
      uint32_t m = (uint32_t)(j - i);
      HIPCHK(ctx, dev.hc.h_in.ensure(bytes + 16 * (size_t)m + 64));
      uint8_t* st = dev.hc.h_in.as<uint8_t>();
      std::vector<uint64_t> soff(m), slen(m);
      uint64_t pos = 0;
      for (uint32_t k = 0; k < m; k++) {
        soff[k] = pos;
        slen[k] = len[i + k];
        memcpy(st + pos, buf + off[i + k], slen[k]);
        memset(st + pos + slen[k], 0, 8);
        pos += (slen[k] + 15) & ~7ull;
      }
      HIPCHK(ctx, dev.hc.bytes.ensure(pos + 64));
      HIPCHK(ctx, dev.hc.off.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.len.ensure(8 * (size_t)m));
      HIPCHK(ctx, dev.hc.out2.ensure(32 * (size_t)m));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.bytes.p, st, pos, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.off.p, soff.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.len.p, slen.data(), 8 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, mvk::launch_blake2b(ctx->kn, dev.hc.bytes.as<uint8_t>(), dev.hc.off.as<uint64_t>(), dev.hc.len.as<uint64_t>(), m,
                                      dev.hc.out2.as<uint8_t>(), dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(out + 32 * i, dev.hc.out2.p, 32 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipStreamSynchronize(dev.stream));
      i = j;
    }
    return MV_OK;
  });
}

mv_status mv_ed25519_verify(mv_ctx* ctx, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk,
                            const uint32_t* key_idx, uint32_t n, uint8_t* status) {
  if (!ctx || (n && (!msg || !sig || !status || (!pk == !key_idx))))
    return set_err(ctx, MV_E_INVALID_ARG, "bad verify args: exactly one of pk / key_idx");
  std::unique_lock<std::mutex> lk(ctx->mu);
  if (key_idx) {
    if (!ctx->has_committee) return set_err(ctx, MV_E_NO_COMMITTEE, "key_idx given but no committee set");
    for (uint32_t i = 0; i < n; i++)
      if (key_idx[i] >= ctx->committee.size()) return set_err(ctx, MV_E_INVALID_ARG, "key_idx out of range");
  }
  const bool pinned = n && host_pinned(msg) && host_pinned(sig) && host_pinned(pk ? (const void*)pk : key_idx);
  for (Device& d : ctx->devs) {
    HIPCHK(ctx, hipSetDevice(d.id));
    reap_idle(ctx, d);
  }
  // Pinned inputs (mv_host_alloc) of a large call stream: chunked DMA copies gate k_bv_prep
  // chunk by chunk (verify_host_streamed). The enqueue holds ctx->mu; the wait for the verdicts
  // does not, so concurrent callers' calls overlap (one's copies beside another's MSM; the
  // reference verifies in one task per peer, net_sync.rs:214-221). (Pageable inputs: one direct
  // H2D per max_batch below; a chunked pack into pinned staging and k_bv_prep reading pinned
  // inputs over PCIe measured slower and were removed in round 6)
  const bool streamed = pinned && !(ctx->flags & MV_FLAG_NO_BATCH);
  if (streamed) {
    const size_t nd = ctx->devs.size();
    std::vector<uint64_t> cut(nd + 1);
    for (size_t d = 0; d <= nd; d++) cut[d] = nd == 1 || n < 2 * 256 ? (d ? n : 0) : (uint64_t)n * d / nd;
    bool big = true;
    for (size_t d = 0; d < nd; d++) big &= cut[d + 1] == cut[d] || cut[d + 1] - cut[d] > 8ull * MV_BATCH_MIN;
    if (big) {
      // one staging slot per device for this call (wait while another call holds them all)
      std::vector<int> slot(nd, -1);
      auto free_slot = [&](Device& d) {
        for (int k = 0; k < Device::kSigCalls; k++)
          if (!d.pin.sig_busy[k]) return k;
        return -1;
      };
      ctx->sig_cv.wait(lk, [&] {
        for (Device& d : ctx->devs)
          if (free_slot(d) < 0) return false;
        return true;
      });
      for (size_t d = 0; d < nd; d++) {
        slot[d] = free_slot(ctx->devs[d]);
        ctx->devs[d].pin.sig_busy[slot[d]] = true;
      }
      mv_status rc = for_each_cut(ctx, cut, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
        HIPCHK(ctx, hipSetDevice(dev.id));
        return verify_host_streamed(ctx, dev, msg, sig, pk, key_idx, lo, hi, slot[&dev - ctx->devs.data()]);
      });
      lk.unlock();
      // wait for this call's batches alone (events, not stream drains: another caller's batches
      // may follow on the same streams), then copy the verdicts out
      std::vector<hipError_t> werr(nd, hipSuccess);
      for (size_t d = 0; d < nd; d++) {
        if (cut[d + 1] == cut[d]) continue;
        Device& dev = ctx->devs[d];
        (void)hipSetDevice(dev.id);
        for (int k = 0; k < 2 && werr[d] == hipSuccess; k++) werr[d] = hipEventSynchronize(dev.pin.sig_done[slot[d]][k]);
        if (rc == MV_OK && werr[d] == hipSuccess)
          memcpy(status + cut[d], dev.pin.sig_stage[slot[d]].p, cut[d + 1] - cut[d]);
      }
      lk.lock();
      for (size_t d = 0; d < nd; d++) {
        Device& dev = ctx->devs[d];
        if (rc != MV_OK || werr[d] != hipSuccess) {  // drain what was queued before the slot is reused
          (void)hipSetDevice(dev.id);
          (void)hipStreamSynchronize(dev.stream);
          for (hipStream_t ps : dev.pin.pstream) (void)hipStreamSynchronize(ps);
        }
        dev.pin.sig_busy[slot[d]] = false;
        if (cut[d + 1] > cut[d]) {
          (void)hipSetDevice(dev.id);
          poll_flags(ctx, dev);
        }
      }
      ctx->sig_cv.notify_all();
      if (rc != MV_OK) return rc;
      for (size_t d = 0; d < nd; d++)
        if (werr[d] != hipSuccess)
          return set_err(ctx, MV_E_HIP, std::string("streamed verify: ") + hipGetErrorString(werr[d]));
      return MV_OK;
    }
  }
  return for_each_shard(ctx, n, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
    HIPCHK(ctx, hipSetDevice(dev.id));
    for (uint64_t i = lo; i < hi; i += ctx->max_batch) {
      uint32_t m = (uint32_t)std::min<uint64_t>(ctx->max_batch, hi - i);
      HIPCHK(ctx, dev.hc.msg.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.sig.ensure(64 * (size_t)m));
      HIPCHK(ctx, dev.hc.status.ensure(m));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.msg.p, msg + 32 * i, 32 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.sig.p, sig + 64 * i, 64 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      const uint8_t* dpk;
      const uint32_t* dki = nullptr;
      if (pk) {
        HIPCHK(ctx, dev.hc.pk.ensure(32 * (size_t)m));
        HIPCHK(ctx, hipMemcpyAsync(dev.hc.pk.p, pk + 32 * i, 32 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
        dpk = dev.hc.pk.as<uint8_t>();
      } else {
        HIPCHK(ctx, dev.hc.keyidx.ensure(4 * (size_t)m));
        HIPCHK(ctx, hipMemcpyAsync(dev.hc.keyidx.p, key_idx + i, 4 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
        dpk = dev.tab.committee_pk.as<uint8_t>();
        dki = dev.hc.keyidx.as<uint32_t>();
      }
      if (!(ctx->flags & MV_FLAG_NO_BATCH) && m >= MV_BATCH_MIN) {
        mv_status st = enqueue_batch(ctx, dev, dev.hc.msg.as<uint8_t>(), dev.hc.sig.as<uint8_t>(), dpk, dki, m,
                                     dev.hc.status.as<uint8_t>(), dev.stream, nullptr);
        if (st != MV_OK) return st;
      } else if (dki) {
        mv_status st = enqueue_committee_verify(ctx, dev, dev.hc.msg.as<uint8_t>(), dev.hc.sig.as<uint8_t>(), dki, m,
                                                dev.hc.status.as<uint8_t>(), dev.stream);
        if (st != MV_OK) return st;
      } else {
        mv_status st = enqueue_verify(ctx, dev, dev.hc.msg.as<uint8_t>(), dev.hc.sig.as<uint8_t>(), dpk, nullptr, m,
                                      dev.hc.status.as<uint8_t>(), dev.stream);
        if (st != MV_OK) return st;
      }
      HIPCHK(ctx, hipMemcpyAsync(status + i, dev.hc.status.p, m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipStreamSynchronize(dev.stream));
      poll_flags(ctx, dev);
    }
    return MV_OK;
  });
}

mv_status mv_ed25519_sign(mv_ctx* ctx, const uint8_t* seed, const uint8_t* msg, uint32_t n, uint8_t* pk,
                          uint8_t* sig) {
  if (!ctx || (n && (!seed || !msg || !pk || !sig))) return set_err(ctx, MV_E_INVALID_ARG, "bad sign args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  return for_each_shard(ctx, n, [&](Device& dev, uint64_t lo, uint64_t hi) -> mv_status {
    HIPCHK(ctx, hipSetDevice(dev.id));
    for (uint64_t i = lo; i < hi; i += ctx->max_batch) {
      uint32_t m = (uint32_t)std::min<uint64_t>(ctx->max_batch, hi - i);
      HIPCHK(ctx, dev.hc.msg.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.bytes.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.pk.ensure(32 * (size_t)m));
      HIPCHK(ctx, dev.hc.sig.ensure(64 * (size_t)m));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.bytes.p, seed + 32 * i, 32 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(dev.hc.msg.p, msg + 32 * i, 32 * (size_t)m, hipMemcpyHostToDevice, dev.stream));
      HIPCHK(ctx, mvk::launch_sign(dev.hc.bytes.as<uint8_t>(), dev.hc.msg.as<uint8_t>(), m, dev.tab.btab.p,
                                   dev.hc.pk.as<uint8_t>(), dev.hc.sig.as<uint8_t>(), dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(pk + 32 * i, dev.hc.pk.p, 32 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipMemcpyAsync(sig + 64 * i, dev.hc.sig.p, 64 * (size_t)m, hipMemcpyDeviceToHost, dev.stream));
      HIPCHK(ctx, hipStreamSynchronize(dev.stream));
    }
    return MV_OK;
  });
}

mv_status mv_online_stats(mv_ctx* ctx, uint64_t* requests, uint64_t* launches) {
  if (!ctx) return MV_E_INVALID_ARG;
  uint64_t r = 0, l = 0;
  for (auto& dev : ctx->devs)
    if (dev.online) {
      r += dev.online->requests.load();
      l += dev.online->launches.load();
    }
  if (requests) *requests = r;
  if (launches) *launches = l;
  return MV_OK;
}

mv_status mv_queue_stats(mv_ctx* ctx, uint64_t* calls, uint64_t* passes) {
  if (!ctx) return MV_E_INVALID_ARG;
  if (calls) *calls = ctx->q_calls.load();
  if (passes) *passes = ctx->q_passes.load();
  return MV_OK;
}

mv_status mv_dev_ed25519_verify(mv_ctx* ctx, int device, const uint8_t* d_msg, const uint8_t* d_sig,
                                const uint8_t* d_pk, uint32_t n, uint8_t* d_status, void* stream) {
  if (!ctx || (n && (!d_msg || !d_sig || !d_pk || !d_status))) return set_err(ctx, MV_E_INVALID_ARG, "bad args");
  if ((((uintptr_t)d_msg) | ((uintptr_t)d_sig) | ((uintptr_t)d_pk)) & 15)
    return set_err(ctx, MV_E_INVALID_ARG, "device inputs must be 16-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  return enqueue_verify(ctx, *dev, d_msg, d_sig, d_pk, nullptr, n, d_status, s);
}

mv_status mv_dev_ed25519_verify_batch(mv_ctx* ctx, int device, const uint8_t* d_msg, const uint8_t* d_sig,
                                      const uint8_t* d_pk, const uint32_t* d_key_idx, uint32_t n,
                                      uint8_t* d_status, uint32_t* d_batch_ok, void* stream) {
  if (!ctx || (n && (!d_msg || !d_sig || !d_pk || !d_status))) return set_err(ctx, MV_E_INVALID_ARG, "bad args");
  if ((((uintptr_t)d_msg) | ((uintptr_t)d_sig) | ((uintptr_t)d_pk)) & 15)
    return set_err(ctx, MV_E_INVALID_ARG, "device inputs must be 16-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev->id));
  reap_idle(ctx, *dev);
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  return enqueue_batch(ctx, *dev, d_msg, d_sig, d_pk, d_key_idx, n, d_status, s, d_batch_ok, nullptr, true);
}

mv_status mv_batch_counters(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return MV_E_INVALID_ARG;
  mv_status st = mv_batch_stats(ctx, out, out + 1);
  out[2] = ctx->groups_run.load();
  out[3] = ctx->groups_failed.load();
  return st;
}

mv_status mv_batch_routes(mv_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return MV_E_INVALID_ARG;
  mv_status st = mv_batch_stats(ctx, out, nullptr);  // accounts every completed batch first
  out[1] = ctx->single_batches.load();
  out[2] = ctx->dense_failures.load();
  return st;
}

mv_status mv_set_batch_groups(mv_ctx* ctx, uint32_t groups) {
  if (!ctx || groups > (uint32_t)mvk::BATCH_MAX_GROUPS) return set_err(ctx, MV_E_INVALID_ARG, "groups > 16");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->groups_fixed = groups;
  ctx->guard_left = 0;  // a new policy starts unguarded
  ctx->single_left = 0;
  return MV_OK;
}

mv_status mv_set_stage_timing(mv_ctx* ctx, int enable) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->stage_timing = enable != 0;
  return MV_OK;
}

mv_status mv_stage_times(mv_ctx* ctx, double* ms, uint64_t* calls, int reset) {
  if (!ctx) return MV_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(ctx->tmu);
  for (auto& pe : ctx->pending) {
    HIPCHK(ctx, hipSetDevice(pe.device));
    mvr::EventSet& ev = pe.events;
    HIPCHK(ctx, hipEventSynchronize(ev.back()));
    for (size_t i = 0; i + 1 < ev.size(); i++) {
      float t = 0;
      HIPCHK(ctx, hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      ctx->stage_ms[pe.first_stage + i] += t;
      ctx->stage_calls[pe.first_stage + i]++;
    }
    ev.release();
  }
  ctx->pending.clear();
  for (int i = 0; i < MV_NSTAGES; i++) {
    if (ms) ms[i] = ctx->stage_ms[i];
    if (calls) calls[i] = ctx->stage_calls[i];
  }
  if (reset) {
    for (double& x : ctx->stage_ms) x = 0;
    for (uint64_t& x : ctx->stage_calls) x = 0;
  }
  return MV_OK;
}

mv_status mv_batch_stats(mv_ctx* ctx, uint64_t* batches, uint64_t* fallbacks) {
  if (!ctx) return MV_E_INVALID_ARG;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto& dev : ctx->devs) {
      (void)hipSetDevice(dev.id);
      poll_flags(ctx, dev);
    }
  }
  if (batches) *batches = ctx->batches.load();
  if (fallbacks) *fallbacks = ctx->fallbacks.load();
  return MV_OK;
}

mv_status mv_dev_ed25519_sign(mv_ctx* ctx, int device, const uint8_t* d_seed, const uint8_t* d_msg, uint32_t n,
                              uint8_t* d_pk, uint8_t* d_sig, void* stream) {
  if (!ctx || (n && (!d_seed || !d_msg || !d_pk || !d_sig))) return set_err(ctx, MV_E_INVALID_ARG, "bad args");
  if ((((uintptr_t)d_seed) | ((uintptr_t)d_msg) | ((uintptr_t)d_pk) | ((uintptr_t)d_sig)) & 15)
    return set_err(ctx, MV_E_INVALID_ARG, "device buffers must be 16-byte aligned");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device* dev = find_dev(ctx, device);
  if (!dev) return set_err(ctx, MV_E_NO_DEVICE, "device not in context");
  HIPCHK(ctx, hipSetDevice(dev->id));
  hipStream_t s = stream ? (hipStream_t)stream : dev->stream;
  HIPCHK(ctx, mvk::launch_sign(d_seed, d_msg, n, dev->tab.btab.p, d_pk, d_sig, s));
  return MV_OK;
}

mv_status mv_selftest(mv_ctx* ctx, int op, const uint32_t* in, uint32_t n, uint32_t* out) {
  if (!ctx || (n && (!in || !out))) return set_err(ctx, MV_E_INVALID_ARG, "bad selftest args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  HIPCHK(ctx, hipSetDevice(dev.id));
  const bool wide = op >= mvk::SELFTEST_WIDE_OP;
  const size_t row = wide ? 256 : 64;  // bytes per row, in and out
  HIPCHK(ctx, dev.hc.bytes.ensure(row * n + 64));
  HIPCHK(ctx, dev.hc.out2.ensure(row * n + 64));
  HIPCHK(ctx, hipMemcpyAsync(dev.hc.bytes.p, in, row * n, hipMemcpyHostToDevice, dev.stream));
  if (wide)
    HIPCHK(ctx, mvk::launch_selftest_wide(op, dev.hc.bytes.as<uint32_t>(), n, dev.hc.out2.as<uint32_t>(), dev.stream));
  else
    HIPCHK(ctx, mvk::launch_selftest(op, dev.hc.bytes.as<uint32_t>(), n, dev.tab.btab.p, dev.hc.out2.as<uint32_t>(), dev.stream));
  HIPCHK(ctx, hipMemcpyAsync(out, dev.hc.out2.p, row * n, hipMemcpyDeviceToHost, dev.stream));
  HIPCHK(ctx, hipStreamSynchronize(dev.stream));
  return MV_OK;
}

mv_status mv_selftest_batch_prep(mv_ctx* ctx, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk,
                                 const uint32_t* key_idx, uint32_t n, uint32_t groups, const uint8_t* key,
                                 uint32_t launch_sigs, uint32_t* scal, uint32_t* pts, uint64_t* bsum,
                                 uint8_t* status, uint32_t* info) {
  if (!ctx || !key || !bsum || !info || (n && (!msg || !sig || !scal || !pts || !status || (!pk == !key_idx))))
    return set_err(ctx, MV_E_INVALID_ARG, "bad batch prep args: exactly one of pk / key_idx");
  if (launch_sigs % 256) return set_err(ctx, MV_E_INVALID_ARG, "launch_sigs must be a multiple of 256");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  if (key_idx) {
    if (!ctx->has_committee || !dev.committee_loaded)
      return set_err(ctx, MV_E_NO_COMMITTEE, "key_idx given but no committee set");
    for (uint32_t i = 0; i < n; i++)
      if (key_idx[i] >= ctx->committee.size()) return set_err(ctx, MV_E_INVALID_ARG, "key_idx out of range");
  }
  info[0] = info[1] = info[2] = 0;
  memset(bsum, 0, sizeof(uint64_t) * 12 * mvk::BATCH_MAX_GROUPS);
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev.id));
  // buffers of this call alone (released on return): the engine's own scratch, its counters, the
  // call counter, the guard and the route stay as they are
  constexpr size_t kPtRow = 128, kScRow = 48;
  const size_t bsum_bytes = sizeof(uint64_t) * 12 * mvk::BATCH_MAX_GROUPS;
  mvr::DevBuf d_msg, d_sig, d_pk, d_pts, d_scal, d_bsum, d_status;
  mvr::Event ready;
  HIPCHK(ctx, d_msg.ensure(32 * (size_t)n));
  HIPCHK(ctx, d_sig.ensure(64 * (size_t)n));
  HIPCHK(ctx, d_pk.ensure((pk ? 32 : 4) * (size_t)n));
  HIPCHK(ctx, d_pts.ensure(2 * kPtRow * (size_t)n));
  HIPCHK(ctx, d_scal.ensure(kScRow * (size_t)n));
  HIPCHK(ctx, d_bsum.ensure(bsum_bytes));
  HIPCHK(ctx, d_status.ensure(n));
  HIPCHK(ctx, ready.ensure());
  hipStream_t s = dev.stream;
  HIPCHK(ctx, hipMemcpyAsync(d_msg.p, msg, 32 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(d_sig.p, sig, 64 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(d_pk.p, pk ? (const void*)pk : key_idx, (pk ? 32 : 4) * (size_t)n, hipMemcpyHostToDevice, s));
  // what the kernel does not write reads back as 0xff.. (unwritten rows show)
  HIPCHK(ctx, hipMemsetAsync(d_pts.p, 0xff, 2 * kPtRow * (size_t)n, s));
  HIPCHK(ctx, hipMemsetAsync(d_scal.p, 0xff, kScRow * (size_t)n, s));
  HIPCHK(ctx, hipMemsetAsync(d_status.p, 0xff, n, s));
  HIPCHK(ctx, hipMemsetAsync(d_bsum.p, 0xff, bsum_bytes, s));
  uint32_t kw[10];
  memcpy(kw, key, 40);
  // launch_sigs > 0: the chunked launches of the pinned path (one per copy chunk, behind its event)
  std::vector<uint32_t> ends;
  std::vector<hipEvent_t> evs;
  if (launch_sigs)
    for (uint64_t o = launch_sigs;; o += launch_sigs) {
      ends.push_back((uint32_t)std::min<uint64_t>(o, n));
      evs.push_back(ready);
      if (o >= n) break;
    }
  HIPCHK(ctx, hipEventRecord(ready, s));
  const mvk::ChunkGate gate{evs.data(), (uint32_t)ends.size(), ends.data()};
  const bool com_a = key_idx && !(ctx->flags & MV_FLAG_NO_COMB);
  mvk::BatchPrepInfo pi{};
  HIPCHK(ctx, mvk::launch_batch_prep(ctx->kn, d_msg.as<uint8_t>(), d_sig.as<uint8_t>(),
                                     pk ? d_pk.as<uint8_t>() : dev.tab.committee_pk.as<uint8_t>(),
                                     pk ? nullptr : d_pk.as<uint32_t>(), n, groups, kw, d_pts.p, d_scal.p, d_bsum.p,
                                     d_status.as<uint8_t>(), s, com_a ? dev.tab.combA.p : nullptr,
                                     com_a ? dev.tab.keyok.as<uint8_t>() : nullptr,
                                     com_a ? (uint32_t)ctx->committee.size() : 0u, launch_sigs ? &gate : nullptr, &pi));
  HIPCHK(ctx, hipMemcpyAsync(scal, d_scal.p, kScRow * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(pts, d_pts.p, (pi.a_rows ? 2 : 1) * kPtRow * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(bsum, d_bsum.p, bsum_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(status, d_status.p, n, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  info[0] = pi.groups;
  info[1] = pi.group_sigs;
  info[2] = pi.a_rows;
  return MV_OK;
}

mv_status mv_selftest_batch_msm(mv_ctx* ctx, uint32_t n, uint32_t groups, const uint32_t* scal, const uint32_t* pts,
                                const uint64_t* bsum, const uint32_t* key_idx, uint32_t n_keys, uint32_t* win,
                                uint32_t* asum, uint32_t* flags, uint32_t* info) {
  if (!ctx || !bsum || !win || !asum || !flags || !info || (n && (!scal || !pts)))
    return set_err(ctx, MV_E_INVALID_ARG, "bad batch msm args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  if (key_idx) {
    if (!ctx->has_committee || !dev.committee_loaded || (ctx->flags & MV_FLAG_NO_COMB))
      return set_err(ctx, MV_E_NO_COMMITTEE, "key_idx given but no committee with comb tables set");
    if (n_keys == 0 || n_keys > ctx->committee.size() || n_keys > 512 || ctx->kn.no_key_agg)
      return set_err(ctx, MV_E_INVALID_ARG, "per-key form: 1..512 keys of the committee, MV_NO_KEY_AGG off");
    for (uint32_t i = 0; i < n; i++)
      if (key_idx[i] >= n_keys) return set_err(ctx, MV_E_INVALID_ARG, "key_idx out of range");
  }
  // the bucket keys of a larger scalar would leave the key space (k_bv_prep never writes one)
  for (uint32_t i = 0; i < n; i++)
    if ((scal[12 * (size_t)i + 3] >> 31) || (scal[12 * (size_t)i + 11] >> 29))
      return set_err(ctx, MV_E_INVALID_ARG, "scal: z < 2^127 and z k < 2^253");
  info[0] = info[1] = info[2] = 0;
  if (n == 0) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev.id));
  // buffers of this call alone (released on return), as mv_selftest_batch_prep's
  const uint32_t gs = mvk::batch_group_size(n, groups), ng = (n + gs - 1) / gs;
  const size_t bytes = mvk::batch_scratch_bytes(n, ng);
  mvr::DevBuf d_scr, d_ki;
  HIPCHK(ctx, d_scr.ensure(bytes));
  hipStream_t s = dev.stream;
  if (key_idx) {
    HIPCHK(ctx, d_ki.ensure(4 * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(d_ki.p, key_idx, 4 * (size_t)n, hipMemcpyHostToDevice, s));
  }
  mvk::BatchMsmInfo mi{};
  HIPCHK(ctx, mvk::launch_batch_msm(ctx->kn, n, groups, scal, pts, bsum, key_idx ? d_ki.as<uint32_t>() : nullptr, n_keys,
                                    key_idx ? dev.tab.combA.p : nullptr, dev.tab.combB.p, d_scr.p, bytes, s, &mi));
  constexpr size_t kP3Row = 144;
  HIPCHK(ctx, hipMemcpyAsync(win, mi.win, kP3Row * mi.groups * mi.nw, hipMemcpyDeviceToHost, s));
  if (mi.asum) HIPCHK(ctx, hipMemcpyAsync(asum, mi.asum, kP3Row * mi.groups, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(flags, mi.flag, 4 * (size_t)(1 + mi.groups), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  info[0] = mi.groups;
  info[1] = mi.group_sigs;
  info[2] = mi.nw;
  return MV_OK;
}

mv_status mv_selftest_comb_table(mv_ctx* ctx, int key, uint32_t* out) {
  if (!ctx || !out) return set_err(ctx, MV_E_INVALID_ARG, "bad comb table args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  Device& dev = ctx->devs[0];
  const void* src = dev.tab.combB.p;
  const size_t bytes = mvk::comb_table_bytes(1);
  if (key >= 0) {
    if (!ctx->has_committee || !dev.committee_loaded) return set_err(ctx, MV_E_NO_COMMITTEE, "no committee set");
    if ((size_t)key >= ctx->committee.size()) return set_err(ctx, MV_E_INVALID_ARG, "key outside the committee");
    src = static_cast<const char*>(dev.tab.combA.p) + bytes * (size_t)key;
  }
  HIPCHK(ctx, hipSetDevice(dev.id));
  HIPCHK(ctx, hipStreamSynchronize(dev.stream));  // the tables are built on this stream
  HIPCHK(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, dev.stream));
  HIPCHK(ctx, hipStreamSynchronize(dev.stream));
  return MV_OK;
}

}  // extern "C"
