// libmysti_verify.so: the resident online service of mv_verify_blocks.
#include <limits.h>
#include <linux/futex.h>
#include <sched.h>
#include <stdio.h>
#include <string.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>

#include "engine_internal.h"

using namespace mvi;

// ---- the resident online service (kernels.h k_online) -------------------------------------
// One per device, made on the first eligible request. Page-locked coherent host memory holds
// the control words, the request ring and each slot's bincode in / outputs out (the kernel
// reads and writes them over PCIe, as the launched online path does); device memory holds the
// ticket and each slot's ingest scratch. The kernel runs on its own stream, the engine's only
// one of the highest priority (a queue of its own, so kernels on other streams never wait behind
// it; its 64 workgroups bound its share of the chip), and exits after MV_ONLINE_IDLE_US (default
// 10,000) without a job.

namespace mvi {

int64_t steady_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// Whether a request of n blocks, `bytes` of 8-aligned bincode, takes the online service: the
// calls enqueue_blocks would run as one k_verify_comb16 launch (short blocks, the ingest and
// hash folded in), small enough for one ring slot.
// Long blocks (config-4 shape, ~9.5 KB) take the service too: a request is then one job whose
// A wave hashes the whole pre-image (the R decode runs beside it), against the queue's split
// launch pair: 16 one-block config-4-shape callers 80.8-81.0 k blocks/s, p50 197-198 us, against
// 69.4-70.6 k / 223-225 us (profiles/r04/c5_online_long_r04s.txt). MV_ONLINE_LONG=0: short
// blocks only (< MV_COMB_SPLIT_BYTES on average, as the queue's one-launch case). A block past
// the wave-parallel ingest's LDS window (ingest_dev.h IG_WIN) goes through the queue.
bool online_eligible(mv_ctx* ctx, uint32_t n, uint64_t bytes, uint64_t longest) {
  const mvk::Knobs& kn = ctx->kn;
  if ((ctx->flags & (MV_FLAG_NO_ONLINE | MV_FLAG_NO_COMB | MV_FLAG_HOST_PARSE)) || !kn.online) return false;
  if (n == 0 || n > kOnMax || bytes > kOnInCap) return false;
  if (longest + 32 > mvk::INGEST_WINDOW_BYTES) return false;
  const uint64_t split_bytes = (uint64_t)std::max<int64_t>(0, kn.comb_split_bytes);
  const uint64_t buf_bytes = (bytes + 16 + 15) & ~15ull;
  if (!kn.online_long && split_bytes && buf_bytes >= split_bytes * (uint64_t)n) return false;
  if (!kn.hash_in_comb || !kn.ingest_in_comb) return false;
  return mvk::comb_short_chain(kn, n);
}

void futex_wait_for(std::atomic<uint32_t>& w, uint32_t v, int64_t ns) {
  static_assert(sizeof(std::atomic<uint32_t>) == 4, "futex word");
  timespec ts{(time_t)(ns / 1000000000), (long)(ns % 1000000000)};
  (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&w), FUTEX_WAIT_PRIVATE, v, &ts, nullptr, 0);
}
void futex_wake_all(std::atomic<uint32_t>& w) {
  (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&w), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

// CPUs this process may use: its affinity mask, capped by a cgroup-v2 CPU quota.
int host_cpu_share() {
  cpu_set_t set;
  int n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char quota[32] = {0};
    long period = 0;
    if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
      const long q = atol(quota);
      if (q > 0) n = std::min<int>(n, (int)std::max<long>(1, q / period));
    }
    fclose(f);
  }
  return std::max(1, n);
}

// Wakes the sleeping callers whose done word is set (one thread per service, started with it;
// it polls only while callers sleep and otherwise waits on rcv).
void online_reaper(OnlineSvc* op) {
  OnlineSvc& o = *op;
  std::unique_lock<std::mutex> lk(o.rmu);
  while (!o.rstop) {
    if (o.sleepers.load(std::memory_order_acquire) == 0) {
      o.rcv.wait_for(lk, std::chrono::milliseconds(20));
      continue;
    }
    lk.unlock();
    for (int it = 0; it < 4096 && o.sleepers.load(std::memory_order_relaxed) > 0; it++) {
      for (uint32_t k = 0; k < kOnSlots; k++) {
        uint64_t w = o.sleep_q[k].load(std::memory_order_acquire);
        if (w && __atomic_load_n(&o.ctl->done[k], __ATOMIC_ACQUIRE) == w &&
            o.sleep_q[k].compare_exchange_strong(w, 0, std::memory_order_acq_rel)) {
          o.dwake[k].store(1, std::memory_order_release);
          futex_wake_all(o.dwake[k]);
        }
      }
      __builtin_ia32_pause();
    }
    lk.lock();
  }
}

// Allocations and the stream (o.mu held).
mv_status online_init(mv_ctx* ctx, Device& dev, OnlineSvc& o) {
  if (o.ready) return MV_OK;
  HIPCHK(ctx, hipSetDevice(dev.id));
  const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;
  auto host = [&](HostBuf& b, void** h, void** d, size_t bytes) -> hipError_t {
    hipError_t e = b.ensure(bytes, nullptr, fl);
    if (e != hipSuccess) return e;
    *h = b.p;
    memset(*h, 0, bytes);
    return hipHostGetDevicePointer(d, *h, 0);
  };
  HIPCHK(ctx, host(o.res.ctl, (void**)&o.ctl, &o.ctl_d, sizeof(mvk::OnlineCtl)));
  HIPCHK(ctx, host(o.res.req, (void**)&o.req, &o.req_d, sizeof(mvk::OnlineReq) * kOnSlots));
  HIPCHK(ctx, host(o.res.in, (void**)&o.in, &o.in_d, kOnInStride * kOnSlots));
  HIPCHK(ctx, host(o.res.out, (void**)&o.out, &o.out_d, kOnOutStride * kOnSlots));
  HIPCHK(ctx, o.res.dctl.ensure(sizeof(mvk::OnlineDev)));
  HIPCHK(ctx, hipMemset(o.res.dctl.p, 0, sizeof(mvk::OnlineDev)));
  HIPCHK(ctx, o.res.scr.ensure(mvk::ONLINE_SCR_STRIDE * kOnSlots));
  o.freed.reset(new std::atomic<uint64_t>[kOnSlots]);
  o.dwake.reset(new std::atomic<uint32_t>[kOnSlots]);
  o.sleep_q.reset(new std::atomic<uint64_t>[kOnSlots]);
  o.fseq.reset(new std::atomic<uint32_t>[kOnSlots]);
  o.fwait.reset(new std::atomic<uint32_t>[kOnSlots]);
  for (uint32_t k = 0; k < kOnSlots; k++) {
    o.freed[k].store(0);
    o.dwake[k].store(0);
    o.sleep_q[k].store(0);
    o.fseq[k].store(0);
    o.fwait[k].store(0);
  }
  o.max_spinners = ctx->kn.online_spinners > 0 ? (int)ctx->kn.online_spinners
                                               : std::max(1, host_cpu_share() / 4);
  if (!o.reaper.joinable()) {
    o.rstop = false;
    o.reaper = std::thread(online_reaper, &o);
  }
  // The service's stream needs a hardware queue of its own: a kernel queued behind the resident
  // one on a shared queue would wait for it. A stream of the highest priority (the runtime keeps
  // a queue per priority level, and the engine's other streams are all of the default
  // priority). Round 4 used a CU-masked stream: tearing one down left a later hipStreamDestroy
  // of an unrelated stream waiting forever on a runtime lock in about 1 of 10 processes
  // (the driver's round-4 smoke); that form was removed in round 6.
  // MV_ONLINE_PRIO = 0: an ordinary stream (shares a queue; A/B only).
  if (ctx->kn.online_prio) {
    int least = 0, greatest = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(ctx, o.res.stream.create_with_priority(hipStreamNonBlocking, greatest));
  } else {
    HIPCHK(ctx, o.res.stream.create());
  }
  HIPCHK(ctx, o.res.exited.ensure());
  o.trace = ctx->kn.online_trace != 0;
  o.debug = ctx->kn.online_debug != 0;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev.id) == hipSuccess && khz > 0)
      o.ticks_per_us = khz / 1000.0;
    else
      (void)hipGetLastError();
  }
  const int64_t ge = ctx->kn.online_wgs;  // resident workgroups (4-block jobs in flight; 0: 64)
  o.grid = (uint32_t)(ge > 0 ? std::max<int64_t>(2, ge) : 64);  // >= 2: the poller + workers
  o.grid = std::min<uint32_t>(o.grid, mvk::ONLINE_MAX_WGS);
  o.ready = true;
  return MV_OK;
}

// Launches the kernel unless one is live (o.mu held).
mv_status online_ensure_running(mv_ctx* ctx, Device& dev, OnlineSvc& o) {
  if (o.launched) {
    // the poller's liveness word (comb.hip k_online): the launch number while it runs,
    // | ONLINE_WG_LEFT once it has left -- no runtime query on the request path. An older
    // value means the launch has not started yet: it will see the request.
    const uint32_t w = __atomic_load_n(&o.ctl->wg[0], __ATOMIC_ACQUIRE);
    if (w != (o.launch_no | mvk::ONLINE_WG_LEFT)) return MV_OK;
  }
  if (ctx->kn.online_inject) {  // fault injection (tests): the launch fails
    (void)hipGetLastError();
    return set_err(ctx, MV_E_HIP, "online service: injected launch failure (MV_ONLINE_INJECT)");
  }
  if (o.launched) {
    const hipError_t q = hipEventQuery(o.res.exited);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();
      return MV_OK;  // still running
    }
    if (q != hipSuccess) {
      o.failed = true;
      return set_err(ctx, MV_E_HIP, std::string("online service: ") + hipGetErrorString(q));
    }
  }
  const uint64_t idle_us = (uint64_t)std::max<int64_t>(0, ctx->kn.online_idle_us);
  o.idle_us = idle_us;
  __atomic_store_n(&o.ctl->stop, 0ull, __ATOMIC_RELEASE);
  HIPCHK(ctx, hipSetDevice(dev.id));
  // the kernel's wall clock (s_memrealtime) in kHz; a launch lives at most 60 s (callers relaunch)
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev.id) != hipSuccess || khz <= 0) {
    (void)hipGetLastError();
    khz = 100000;
  }
  const uint64_t per_us = (uint64_t)khz / 1000 ? (uint64_t)khz / 1000 : 1;
  mvk::OnlineArgs a{};
  a.ctl = (mvk::OnlineCtl*)o.ctl_d;
  a.reqs = (const mvk::OnlineReq*)o.req_d;
  a.dev = o.res.dctl.as<mvk::OnlineDev>();
  a.in_host = static_cast<const uint8_t*>(o.in_d);
  a.out_host = static_cast<uint8_t*>(o.out_d);
  a.scr = o.res.scr.as<uint8_t>();
  a.combB = dev.tab.combB.p;
  a.combA = dev.tab.combA.p;
  a.key_ok = dev.tab.keyok.as<uint8_t>();
  a.pk = dev.tab.committee_pk.as<uint8_t>();
  a.stakes = dev.tab.stakes.as<uint64_t>();
  const mvh::Committee& com = ctx->committee;  // fixed while the launch lives (mv_set_committee stops it)
  a.epoch = com.epoch;
  a.quorum_thr = com.quorum_threshold;
  a.n_auth = (uint32_t)com.size();
  a.launch = ++o.launch_no;
  a.idle_ticks = idle_us * per_us;
  a.max_ticks = 60000000ull * per_us;
  HIPCHK(ctx, mvk::launch_online(a, o.grid, o.res.stream));
  if (o.debug)
    fprintf(stderr, "[online] launch %u: grid %u, idle %llu us, wall clock %d kHz\n", a.launch, o.grid,
            (unsigned long long)idle_us, khz);
  HIPCHK(ctx, hipEventRecord(o.res.exited, o.res.stream));
  o.launched = true;
  o.launches++;
  return MV_OK;
}

// Polls ev until it completes or limit_ms pass (no blocking runtime wait, which cannot be
// bounded); true once complete.
bool event_done_within(hipEvent_t ev, int64_t limit_ms) {
  const int64_t t0 = steady_ns();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return true;
    (void)hipGetLastError();
    if (q != hipErrorNotReady) return true;  // an error: nothing more will complete on it
    if (steady_ns() - t0 > limit_ms * 1000000) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// The service's state words, for a launch that does not end in time (stderr).
void online_dump(const OnlineSvc& o, const char* why) {
  const mvk::OnlineCtl* c = o.ctl;
  uint32_t running = 0, left = 0, other = 0;
  std::string stuck;
  for (uint32_t g = 0; g < o.grid && g < mvk::ONLINE_MAX_WGS; g++) {
    const uint32_t w = __atomic_load_n(&c->wg[g], __ATOMIC_ACQUIRE);
    if (w == o.launch_no) {
      running++;
      if (stuck.size() < 96) stuck += " " + std::to_string(g);
    } else if (w == (o.launch_no | mvk::ONLINE_WG_LEFT)) {
      left++;
    } else {
      other++;
    }
  }
  fprintf(stderr,
          "[online] %s: launch %u grid %u: %u workgroups running (%s), %u left, %u not started; stop %llu tail %llu "
          "next_q %llu; poller exit: why %llu ready %llu jobs_head %llu jobs_tail %llu\n",
          why, o.launch_no, o.grid, running, stuck.empty() ? "-" : stuck.c_str() + 1, left, other,
          (unsigned long long)c->stop, (unsigned long long)c->tail, (unsigned long long)o.next_q,
          (unsigned long long)c->exit_why, (unsigned long long)c->exit_ready, (unsigned long long)c->exit_head,
          (unsigned long long)c->exit_tail);
}

// Stops the kernel once it is idle and waits for it, bounded (o.mu held). The launch's own
// limits end every wave within max_ticks + idle (60 s + MV_ONLINE_IDLE_US); a launch still
// running well past that is reported (online_dump) and the service is left stuck: its memory is
// then never freed (the kernel may still touch it). Returns false in that case.
bool online_stop(OnlineSvc& o) {
  if (!o.ready || !o.launched) return true;
  __atomic_store_n(&o.ctl->stop, 1ull, __ATOMIC_RELEASE);
  bool done = event_done_within(o.res.exited, 2000);
  if (!done) {
    online_dump(o, "stop: no exit after 2 s");
    done = event_done_within(o.res.exited, 70000);
    if (!done) online_dump(o, "stop: no exit after 72 s, service abandoned");
  }
  if (!done) {
    o.failed = o.stuck = true;
    return false;
  }
  __atomic_store_n(&o.ctl->stop, 0ull, __ATOMIC_RELEASE);
  o.launched = false;
  return true;
}

void online_release(OnlineSvc& o) {
  if (o.reaper.joinable()) {
    {
      std::lock_guard<std::mutex> lk(o.rmu);
      o.rstop = true;
    }
    o.rcv.notify_all();
    o.reaper.join();
  }
  if (!online_stop(o)) {  // stuck: its stream and memory are left alone, whoever destroys o
    o.res.abandon();
    return;
  }
  if (o.trace && o.tr_n) {
    const double n = (double)o.tr_n;
    fprintf(stderr,
            "[online] %llu requests, mean us: host publish->done seen %.1f | kernel: seen->ready %.1f, "
            "ready->claim %.1f, claim->done %.1f, seen->done %.1f | job 0 from its claim: barrier 0 %.1f, "
            "B rows %.1f, S %.1f, R decoded %.1f, barrier 1 %.1f, verdict %.1f, fenced %.1f, digests %.1f, "
            "k %.1f\n",
            (unsigned long long)o.tr_n, o.tr_sum[0] / n, o.tr_sum[1] / n, o.tr_sum[2] / n, o.tr_sum[3] / n,
            o.tr_sum[4] / n, o.tr_sum[5] / n, o.tr_sum[6] / n, o.tr_sum[7] / n, o.tr_sum[8] / n, o.tr_sum[9] / n,
            o.tr_sum[10] / n, o.tr_sum[11] / n, o.tr_sum[12] / n, o.tr_sum[13] / n);
  }
  mvr::reset(o.res);
  o.ctl = nullptr, o.req = nullptr, o.in = nullptr, o.out = nullptr;
  o.ready = false;
}

// One request through the service: reserve a ring slot, pack the blocks into its page-locked
// input, publish the descriptor, then poll the slot's done word (the caller's thread spins:
// no launch, no event, no wake-up). ctx->com_mu is held shared by the caller.
mv_status online_verify(mv_ctx* ctx, Device& dev, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                        uint32_t n, uint8_t* status, uint8_t* md, uint8_t* bd) {
  OnlineSvc& o = *dev.online;
  uint64_t q;
  {
    std::lock_guard<std::mutex> lk(o.mu);
    if (o.failed) return set_err(ctx, MV_E_HIP, "online service failed earlier");
    mv_status rc = online_init(ctx, dev, o);
    if (rc != MV_OK) {
      o.failed = true;
      return rc;
    }
    q = o.next_q++;
    __atomic_store_n(&o.ctl->tail, o.next_q, __ATOMIC_RELEASE);
    rc = online_ensure_running(ctx, dev, o);
    if (rc != MV_OK) {
      // request q is never published, so the poller would stop at it: the service is done
      // (every later reservation sees `failed`, every waiting caller leaves its loop)
      o.failed = true;
      return rc;
    }
  }
  o.requests++;
  const uint32_t slot = (uint32_t)(q % kOnSlots);
  if (q >= kOnSlots) {  // the slot's previous request must have been read out by its owner
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; o.freed[slot].load(std::memory_order_acquire) != q - kOnSlots + 1; spins++) {
      // the owner of request q - 64 failed (its service failed with it) or never returns
      if (o.failed.load(std::memory_order_relaxed) || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
        o.failed = true;
        return set_err(ctx, MV_E_HIP, "online service failed: ring slot never released");
      }
      if (spins < 256) {
        __builtin_ia32_pause();
        continue;
      }
      // sleep until the owner frees the slot (it wakes fseq's sleepers), 1 ms at most
      const uint32_t seen = o.fseq[slot].load(std::memory_order_acquire);
      o.fwait[slot].fetch_add(1, std::memory_order_acq_rel);
      if (o.freed[slot].load(std::memory_order_acquire) != q - kOnSlots + 1) futex_wait_for(o.fseq[slot], seen, 1000000);
      o.fwait[slot].fetch_sub(1, std::memory_order_acq_rel);
    }
  }
  // the slot's input: off[n] | len[n] | bincode (8-aligned blocks) | 16 zero bytes; the poller
  // copies it to the slot's HBM scratch, which every device pointer below refers to
  uint8_t* in = o.in + kOnInStride * slot;
  uint64_t* hoff = reinterpret_cast<uint64_t*>(in);
  uint64_t* hlen = hoff + n;
  uint8_t* bytes = in + 16 * (size_t)n;
  uint64_t pos = 0;
  for (uint32_t k = 0; k < n; k++) {
    const uint64_t l = len[k];
    hoff[k] = pos;
    hlen[k] = l;
    memcpy(bytes + pos, buf + off[k], l);
    const uint64_t pl = (l + 7) & ~7ull;
    memset(bytes + pos + l, 0, pl - l);
    pos += pl;
  }
  memset(bytes + pos, 0, 16);  // 16 readable zero bytes past the last block
  const uint32_t copy_bytes = (uint32_t)((16 * (size_t)n + pos + 16 + 15) & ~(size_t)15);
  uint8_t* out = o.out + kOnOutStride * slot;
  mvk::OnlineReq& r = o.req[slot];
  r.n = n;
  r.copy_bytes = copy_bytes;
  const int64_t t_pub = o.trace ? steady_ns() : 0;
  __atomic_store_n(&r.seq, q + 1, __ATOMIC_RELEASE);  // the descriptor and the bytes above first
  // wait for the slot's done word, spinning (at most max_spinners callers at once) or asleep
  // until the reaper wakes it; every ~100 us (asleep: 1 ms) check that a kernel is still live
  // (one that exited idle just before this request was published is relaunched)
  auto t_last = std::chrono::steady_clock::now();
  const auto t_start = t_last;
  mv_status rc = MV_OK;
  auto is_done = [&] { return __atomic_load_n(&o.ctl->done[slot], __ATOMIC_ACQUIRE) == q + 1; };
  auto check = [&](std::chrono::steady_clock::time_point now) -> bool {  // false: give up (rc set)
    if (o.debug && now - t_start > std::chrono::milliseconds(500) &&
        (now - t_start) % std::chrono::milliseconds(500) < std::chrono::milliseconds(2)) {
      const uint64_t* tr = o.ctl->trace[slot];
      fprintf(stderr, "[online] q %llu slot %u waiting %.1f ms: done %llu seq %llu tail %llu trace %llu %llu %llu %llu\n",
              (unsigned long long)q, slot,
              std::chrono::duration<double, std::milli>(now - t_start).count(),
              (unsigned long long)__atomic_load_n(&o.ctl->done[slot], __ATOMIC_ACQUIRE),
              (unsigned long long)o.req[slot].seq, (unsigned long long)o.ctl->tail, (unsigned long long)tr[0],
              (unsigned long long)tr[1], (unsigned long long)tr[2], (unsigned long long)tr[3]);
    }
    std::lock_guard<std::mutex> lk(o.mu);
    if (o.failed) {
      rc = set_err(ctx, MV_E_HIP, "online service failed");
      return false;
    }
    rc = online_ensure_running(ctx, dev, o);
    if (rc == MV_OK && o.launched && now - t_start > std::chrono::microseconds(std::max<uint64_t>(o.idle_us, 1000))) {
      // waiting longer than the idle limit: a launch that faulted or was aborted never marks its
      // liveness word LEFT, so ask the runtime about its end as well (fail fast, not after 20 s)
      const hipError_t q = hipEventQuery(o.res.exited);
      if (q == hipErrorNotReady)
        (void)hipGetLastError();
      else if (q != hipSuccess)
        rc = set_err(ctx, MV_E_HIP, std::string("online service: ") + hipGetErrorString(q));
    }
    if (rc == MV_OK && now - t_start > std::chrono::seconds(20))
      rc = set_err(ctx, MV_E_HIP, "online service: request timed out");
    if (rc != MV_OK) {
      o.failed = true;  // the slot may still be written: never reuse the service
      return false;
    }
    return true;
  };
  if (o.spinners.fetch_add(1, std::memory_order_acq_rel) < o.max_spinners) {
    for (uint32_t spins = 0; !is_done();) {
      if (++spins < 64) {
        __builtin_ia32_pause();
        continue;
      }
      spins = 0;
      std::this_thread::yield();
      const auto now = std::chrono::steady_clock::now();
      if (now - t_last < std::chrono::microseconds(100)) continue;
      t_last = now;
      if (!check(now)) break;
    }
    o.spinners.fetch_sub(1, std::memory_order_acq_rel);
  } else {
    o.spinners.fetch_sub(1, std::memory_order_acq_rel);
    o.dwake[slot].store(0, std::memory_order_relaxed);
    o.sleep_q[slot].store(q + 1, std::memory_order_release);
    if (o.sleepers.fetch_add(1, std::memory_order_acq_rel) == 0) {
      std::lock_guard<std::mutex> lk(o.rmu);
      o.rcv.notify_one();
    }
    while (!is_done()) {
      futex_wait_for(o.dwake[slot], 0, 1000000);
      if (is_done()) break;
      const auto now = std::chrono::steady_clock::now();
      if (now - t_last < std::chrono::microseconds(900)) continue;
      t_last = now;
      if (!check(now)) break;
    }
    uint64_t w = q + 1;
    o.sleep_q[slot].compare_exchange_strong(w, 0, std::memory_order_acq_rel);
    o.sleepers.fetch_sub(1, std::memory_order_acq_rel);
  }
  if (rc != MV_OK) return rc;
  if (o.trace) {
    const double host_us = (steady_ns() - t_pub) / 1e3;
    const uint64_t* tr = o.ctl->trace[slot];
    const double k = 1.0 / o.ticks_per_us;
    std::lock_guard<std::mutex> lk(o.tr_mu);
    o.tr_sum[0] += host_us;
    o.tr_sum[1] += (double)(int64_t)(tr[1] - tr[0]) * k;
    o.tr_sum[2] += (double)(int64_t)(tr[2] - tr[1]) * k;
    o.tr_sum[3] += (double)(int64_t)(tr[3] - tr[2]) * k;
    o.tr_sum[4] += (double)(int64_t)(tr[3] - tr[0]) * k;
    for (int i = 0; i < 9; i++) o.tr_sum[5 + i] += (double)(int64_t)(tr[4 + i] - tr[2]) * k;
    o.tr_n++;
  }
  const uint8_t* ho = out;
  for (uint32_t k = 0; k < n; k++) {
    status[k] = ho[64 * kOnMax + k];
    if (md) memcpy(md + 32 * (size_t)k, ho + 32 * (size_t)k, 32);
    if (bd) memcpy(bd + 32 * (size_t)k, ho + 32 * ((size_t)kOnMax + k), 32);
  }
  o.freed[slot].store(q + 1, std::memory_order_release);
  o.fseq[slot].fetch_add(1, std::memory_order_acq_rel);
  if (o.fwait[slot].load(std::memory_order_acquire)) futex_wake_all(o.fseq[slot]);
  return MV_OK;
}

}  // namespace mvi
