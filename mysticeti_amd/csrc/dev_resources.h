// Owning types of the host engine's device resources (host only): growable device / pinned
// buffers, events, streams and the event-ordered scratch ring. Every one is move-only and
// releases what it holds in its destructor, so a struct made of them is freed by destroying (or
// resetting) it, with no list of members to keep in step. A process-wide count of the live
// objects (mv_get_option "MV_LIVE_RESOURCES") lets a test see that a destroyed context left
// nothing behind.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

namespace mvr {

// buffers holding memory, events, streams and entries of the retired list, process-wide
inline std::atomic<int64_t> g_live{0};

// Buffers that grow retire the old allocation instead of freeing it at once (the retired list,
// engine.cpp): the block joins the list with the completion event that guards it, or none.
void retire(void* p, bool host, hipEvent_t guard);

// the size to allocate for `bytes` when `cap` is too small: x1.5 steps, exact on first use
inline size_t grown(size_t cap, size_t bytes) { return std::max<size_t>({bytes, 4096, cap ? cap + cap / 2 : 0}); }

enum MemKind { kDevice, kPinned };

template <MemKind K>
struct Buf {
  void* p = nullptr;
  size_t cap = 0;

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~Buf() { release(); }

  // guard: the completion event of the calls that used the buffer (see the retired list), or
  // null (synchronous host-buffer calls: they had finished when the buffer grows).
  // host_flags: hipHostMalloc flags of a pinned buffer.
  hipError_t ensure(size_t bytes, hipEvent_t guard = nullptr, unsigned host_flags = hipHostMallocDefault) {
    if (bytes <= cap) return hipSuccess;
    const size_t want = grown(cap, bytes);
    if (p) {
      retire(p, K == kPinned, guard);
      forget();
    }
    hipError_t e = alloc(want, host_flags);
    if (e != hipSuccess && want > bytes) {  // the geometric step does not fit: exactly
      (void)hipGetLastError();
      e = alloc(std::max<size_t>(bytes, 4096), host_flags);
    }
    return e;
  }
  void release() {
    if (p) (void)(K == kPinned ? hipHostFree(p) : hipFree(p));
    forget();
  }
  // Gives the memory up without freeing it (a resident kernel that would not end may still
  // touch it): leaked on purpose.
  void abandon() { forget(); }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }

 private:
  hipError_t alloc(size_t bytes, unsigned host_flags) {
    const hipError_t e = K == kPinned ? hipHostMalloc(&p, bytes, host_flags) : hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = bytes;
    g_live++;
    return e;
  }
  void forget() {
    if (p) g_live--;
    p = nullptr;
    cap = 0;
  }
};
using DevBuf = Buf<kDevice>;
using HostBuf = Buf<kPinned>;

// An event made on first use (ensure), without timing.
struct Event {
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(ev_, o.ev_);
    }
    return *this;
  }
  ~Event() { release(); }

  hipError_t ensure() {
    if (ev_) return hipSuccess;
    const hipError_t e = hipEventCreateWithFlags(&ev_, hipEventDisableTiming);
    if (e == hipSuccess) g_live++;
    else ev_ = nullptr;
    return e;
  }
  operator hipEvent_t() const { return ev_; }  // null until ensure()
  void release() {
    if (ev_) (void)hipEventDestroy(ev_);
    abandon();
  }
  void abandon() {
    if (ev_) g_live--;
    ev_ = nullptr;
  }

 private:
  hipEvent_t ev_ = nullptr;
};

// A fixed number of events made together, as the plain array the launchers take (a batch's
// stage-timing events, a pinned-input buffer's per-chunk events).
struct EventSet {
  EventSet() = default;
  EventSet(const EventSet&) = delete;
  EventSet& operator=(const EventSet&) = delete;
  EventSet(EventSet&& o) noexcept : evs_(std::move(o.evs_)) { o.evs_.clear(); }
  EventSet& operator=(EventSet&& o) noexcept {
    if (this != &o) {
      release();
      evs_.swap(o.evs_);
    }
    return *this;
  }
  ~EventSet() { release(); }

  // n events with `flags` unless the set holds n already; all of them or, on an error, none
  hipError_t ensure(size_t n, unsigned flags) {
    if (evs_.size() == n) return hipSuccess;
    release();
    evs_.reserve(n);
    for (size_t k = 0; k < n; k++) {
      hipEvent_t ev = nullptr;
      const hipError_t e = hipEventCreateWithFlags(&ev, flags);
      if (e != hipSuccess) {
        release();
        return e;
      }
      evs_.push_back(ev);
      g_live++;
    }
    return hipSuccess;
  }
  bool empty() const { return evs_.empty(); }
  size_t size() const { return evs_.size(); }
  hipEvent_t* data() { return evs_.data(); }
  hipEvent_t operator[](size_t k) const { return evs_[k]; }
  hipEvent_t back() const { return evs_.back(); }
  void release() {
    for (hipEvent_t ev : evs_) (void)hipEventDestroy(ev);
    g_live -= (int64_t)evs_.size();
    evs_.clear();
  }

 private:
  std::vector<hipEvent_t> evs_;
};

// A stream, made where the engine decides (mv_create makes them all, in a fixed order: the
// runtime hands out its hardware queues in creation order).
struct Stream {
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(s_, o.s_);
    }
    return *this;
  }
  ~Stream() { release(); }

  hipError_t create(unsigned flags = hipStreamNonBlocking) { return made(hipStreamCreateWithFlags(&s_, flags)); }
  hipError_t create_with_priority(unsigned flags, int priority) {
    return made(hipStreamCreateWithPriority(&s_, flags, priority));
  }
  operator hipStream_t() const { return s_; }
  void release() {
    if (s_) (void)hipStreamDestroy(s_);
    abandon();
  }
  void abandon() {
    if (s_) g_live--;
    s_ = nullptr;
  }

 private:
  hipError_t made(hipError_t e) {
    if (e == hipSuccess) g_live++;
    else s_ = nullptr;
    return e;
  }
  hipStream_t s_ = nullptr;
};

// A ring of N scratch slots: consecutive calls rotate over them, so a call on one stream can
// run while the previous ones (on other streams) finish their latency-bound tails; an event per
// slot orders reuse across streams and guards the slot's buffers when they grow.
template <class Scratch, int N>
struct ScratchRing {
  struct Slot {
    Scratch scr;
    Event done;
    bool used = false;
  };
  Slot slot[N];
  int next = 0;

  // The next slot (its event made on first use); the ring moves on.
  hipError_t claim(int* k) {
    *k = next;
    next = (next + 1) % N;
    return slot[*k].done.ensure();
  }
  // Orders stream s behind slot k's last user (device-side only). query_first: no wait when
  // that user has finished already (a cross-stream wait costs a queue drain).
  hipError_t order_behind(int k, hipStream_t s, bool query_first = false) {
    if (!slot[k].used) return hipSuccess;
    if (query_first) {
      if (hipEventQuery(slot[k].done) == hipSuccess) return hipSuccess;
      (void)hipGetLastError();  // hipErrorNotReady is not an error here
    }
    return hipStreamWaitEvent(s, slot[k].done, 0);
  }
  hipError_t take(hipStream_t s, int* k, bool query_first = false) {
    const hipError_t e = claim(k);
    return e != hipSuccess ? e : order_behind(*k, s, query_first);
  }
  // Slot k was claimed but not used: the next call gets it.
  void hand_back(int k) { next = k; }
  // Slot k's user is everything enqueued on s so far.
  hipError_t mark_used(int k, hipStream_t s) {
    const hipError_t e = hipEventRecord(slot[k].done, s);
    if (e == hipSuccess) slot[k].used = true;
    return e;
  }
};

// Releases everything a group of resources holds and returns it to its initial state. Members
// go in declaration order, an array element by element: a ring slot's or a pass set's buffers
// go before its own events and streams, not before every other slot's. Callers reset a group
// only once nothing on the device uses it (mv_destroy: after the device drain).
template <class Group>
void reset(Group& g) {
  g = Group();
}

}  // namespace mvr
