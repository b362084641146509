// What the index kernels share (index.hip, pending.hip, dag_store.hip, decide.hip, linearize.hip,
// propose.hip, votes.hip; replay.hip for the workgroup prefix): the table's slot layout, the item
// record of an insert, the keyed hash, the read-only probe, the claim into a fresh table, the wave
// and workgroup reductions and the compaction pass. The build has no relocatable device code:
// everything here is inline or a template.
//
// Table: open addressing, linear probing, 64-byte slots of eight u64 words
//   [0] tag    0 = empty, else the (truncated) second hash of the key, never 0
//   [1] meta   low half: the state (0 until the slot is filled); high half: the owner word
//   [2..7]     the key: authority, round, four digest words
// Probe start and tag are the two halves of SipHash-2-4-128 of the six key words under the
// context's 128-bit secret: the digests of includes are bytes a peer chooses. No result rests on
// a tag: a match is a match only after all six words compare equal.
//
// Memory model. Inside one launch lanes talk only through agent-scope atomic read-modify-writes
// on single words: CAS on the tag, max on the owner word (which holds ~item, so the lowest item
// wins), max on the state. No lane waits for another, and no kernel compares against key bytes
// that were stored in the same launch: a slot whose state is 0 was claimed in this launch, and
// its key is read only by a later kernel. One insert round is three kernels on one stream:
//   k_ix_claim    probe; a slot filled before this launch (state != 0) is compared in full; the
//                 first empty slot is claimed by CAS; a lane that stops at a slot (claimed now, or
//                 found and to be raised) puts its item into the owner word
//   k_ix_fill     the owner of a claimed slot writes key and state; the owner of a found slot
//                 raises its state; the counters of HAVE and WANTED entries
//   k_ix_settle   a lane that stopped at a slot claimed in this round without owning it compares
//                 in full: equal, it is a duplicate of the owner; different (same tag, other key)
//                 it is marked for another round, which probes on past that slot. Owners clear
//                 the owner word.
// The host runs rounds while the retry counter is not 0 (64-bit tags: never; MV_INDEX_TAG_BITS=2:
// all the time). All items with one key stop at the same slot in a round (tags are set once and
// never cleared), so they share their fate, and the owner among them is the lowest item.
// Every probe loop is bounded by the table size; a probe that runs out sets the error word.
//
// Compaction. A stable "count per workgroup, k_ix_scan, list at the scanned place" pass is one
// functor F through compact_pass (k_compact_count<F>, launch_index_scan, k_compact_list<F>):
//   F::WEIGHTS            1 or 2: a one-weight pass does one wg_excl per kernel and one scan launch
//   weigh(i, &a[, &b])    the item's weights -- 0 / 1 for a flag, or a count such as its includes
//   place(i, a, ra[, b, rb])  the item's weights again and their exclusive ranks over all items
// Every lane of every workgroup calls both, the lanes with i >= n included (their weights are 0):
// the workgroup prefix has barriers, and place() is where a pass does its all-lane extras such as
// wave_count_to. The predicate is stated once, in weigh(); the list kernel hands place() what it
// gave. Items keep their order: the rank of item i is the sum of the weights of the items below i.
// Caps and bounds checks are place()'s own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "block_ref.h"
#include "kernels.h"

namespace mv::ix {

using mvk::IndexKeys;
using mvk::IndexTable;
using mvk::AcceptArrays;
using mvk::DagStore;
using mvk::PendStore;
typedef unsigned long long u64;

constexpr int WG = mvk::IX_WG;
constexpr int SLOT_WORDS = 8;

// an item's record: slot index | prior state << 40 | code << 44 | FRESH
constexpr u64 SLOT_MASK = (1ull << 40) - 1;
constexpr int PRIOR_SHIFT = 40, CODE_SHIFT = 44;
constexpr u64 FRESH = 1ull << 48;  // an owner whose slot's owner word is still set
enum Code : u64 {
  C_NONE = 0,     // not an item (no source)
  C_FOUND = 1,    // matched a slot filled earlier whose state is to be raised
  C_CLAIMED = 2,  // stopped at a slot claimed in this round
  C_NEW = 3,      // owner: created the entry
  C_RAISED = 4,   // owner: raised the entry
  C_DUP = 5,      // same key as an owner of this call
  C_NOOP = 6,     // the entry was there with a state at least as high
  C_RETRY = 7,    // same tag, other key: probes on in the next round
  C_FAIL = 8,     // the probe ran through the whole table
};

__device__ inline u64 pack(u64 slot, uint32_t prior, u64 code) {
  return slot | ((u64)prior << PRIOR_SHIFT) | (code << CODE_SHIFT);
}
__device__ inline u64 code_of(u64 it) { return (it >> CODE_SHIFT) & 15; }
__device__ inline uint32_t prior_of(u64 it) { return (uint32_t)(it >> PRIOR_SHIFT) & 3; }

__device__ inline uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

#define MV_SIPROUND                                  \
  do {                                               \
    v0 += v1, v1 = (v1 << 13) | (v1 >> 51), v1 ^= v0; \
    v0 = (v0 << 32) | (v0 >> 32);                    \
    v2 += v3, v3 = (v3 << 16) | (v3 >> 48), v3 ^= v2; \
    v0 += v3, v3 = (v3 << 21) | (v3 >> 43), v3 ^= v0; \
    v2 += v1, v1 = (v1 << 17) | (v1 >> 47), v1 ^= v2; \
    v2 = (v2 << 32) | (v2 >> 32);                    \
  } while (0)

// SipHash-2-4 with 128-bit output over the 48 key bytes: *start = first half, the tag from the second
__device__ inline void hash_key(const IndexTable& t, const uint64_t k[6], uint64_t* start, uint64_t* tag) {
  uint64_t v0 = t.k0 ^ 0x736f6d6570736575ull, v1 = t.k1 ^ 0x646f72616e646f6dull;
  uint64_t v2 = t.k0 ^ 0x6c7967656e657261ull, v3 = t.k1 ^ 0x7465646279746573ull;
  v1 ^= 0xee;
#pragma unroll
  for (int w = 0; w < 6; w++) {
    v3 ^= k[w];
    MV_SIPROUND;
    MV_SIPROUND;
    v0 ^= k[w];
  }
  const uint64_t b = 48ull << 56;
  v3 ^= b;
  MV_SIPROUND;
  MV_SIPROUND;
  v0 ^= b;
  v2 ^= 0xee;
  for (int r = 0; r < 4; r++) MV_SIPROUND;
  *start = (v0 ^ v1 ^ v2 ^ v3) & t.mask;
  v1 ^= 0xdd;
  for (int r = 0; r < 4; r++) MV_SIPROUND;
  uint64_t g = v0 ^ v1 ^ v2 ^ v3;
  if (t.tag_bits < 64) g &= (1ull << t.tag_bits) - 1;
  *tag = g ? g : 1;
}

__device__ inline const uint8_t* key_ptr(const IndexKeys& ks, uint64_t i) {
  return ks.base + (ks.off ? ks.off[i] : i * ks.stride);
}
__device__ inline void load_key(const IndexKeys& ks, uint64_t i, uint64_t k[6]) {
  const uint8_t* p = key_ptr(ks, i);
#pragma unroll
  for (int w = 0; w < 6; w++) k[w] = ld64(p + (ks.ref ? br::key_word_off(w) : 8 * (uint64_t)w));
}
__device__ inline bool has_src(const IndexKeys& ks, uint64_t i) { return !ks.off || ks.off[i] != mvk::IX_NO_SRC; }

// plain loads: the slot was filled by an earlier kernel
__device__ inline bool key_eq(const u64* slot, const uint64_t k[6]) {
  bool eq = true;
#pragma unroll
  for (int w = 0; w < 6; w++) eq &= slot[2 + w] == k[w];
  return eq;
}
// the six key words of a slot to dst: all loads ahead of the stores (the two may alias for all the compiler knows)
__device__ inline void copy_key(uint64_t* dst, const u64* slot) {
  u64 k[6];
#pragma unroll
  for (int w = 0; w < 6; w++) k[w] = slot[2 + w];
#pragma unroll
  for (int w = 0; w < 6; w++) dst[w] = k[w];
}
__device__ inline uint32_t* meta_of(u64* slot) { return reinterpret_cast<uint32_t*>(slot + 1); }
__device__ inline uint32_t slot_state(const u64* slots, uint64_t p) { return (uint32_t)slots[SLOT_WORDS * p + 1]; }
__device__ inline bool item_has_slot(u64 it) {
  const u64 c = code_of(it);
  return c == C_NEW || c == C_RAISED || c == C_DUP || c == C_NOOP;
}

constexpr u64 DG_NO_SLOT = mvk::DG_NO_SLOT;
__device__ inline uint32_t probe_len(uint64_t dist) { return (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull); }

// Read-only probe: the slot of key k, DG_NO_SLOT without an entry (no table yet, an empty slot met
// first, or -- *fail -- the probe ran through the whole table). Nothing writes the table in a launch
// that calls it. *probe = slots examined, for the callers that report IX_CTL_MAXPROBE.
__device__ inline u64 find_slot(const IndexTable& t, const uint64_t k[6], uint32_t* probe, bool* fail) {
  *probe = 0, *fail = false;
  if (!t.slots) return DG_NO_SLOT;
  uint64_t start, tag;
  hash_key(t, k, &start, &tag);
  uint64_t p = start, dist = 0;
  u64 at = DG_NO_SLOT;
  bool ended = false;
  for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
    const u64* slot = t.slots + SLOT_WORDS * p;
    const u64 g = slot[0];
    if (g == 0) {
      ended = true;
      break;
    }
    if (g == tag && key_eq(slot, k)) {
      at = p;
      ended = true;
      break;
    }
  }
  *probe = probe_len(dist);
  *fail = !ended;
  return at;
}
// the state of key k, MV_REF_ABSENT without an entry
__device__ inline uint32_t lookup(const IndexTable& t, const uint64_t k[6], uint32_t* probe, bool* fail) {
  const u64 p = find_slot(t, k, probe, fail);
  return p == DG_NO_SLOT ? (uint32_t)MV_REF_ABSENT : slot_state(t.slots, p);
}

// An entry into a fresh table whose keys are distinct (a rebuild, a move): the first empty slot is
// claimed by CAS, its key and meta word written, and nothing compares (no key of this launch is
// read). The slot, or DG_NO_SLOT when the probe ran through the whole table; *probe = slots examined.
__device__ inline u64 claim_fresh(const IndexTable& t, const uint64_t k[6], u64 meta, uint32_t* probe) {
  uint64_t start, tag;
  hash_key(t, k, &start, &tag);
  uint64_t p = start, dist = 0;
  u64 at = DG_NO_SLOT;
  for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
    u64* slot = t.slots + SLOT_WORDS * p;
    if (atomicCAS(slot, 0ull, (u64)tag) != 0) continue;
#pragma unroll
    for (int w = 0; w < 6; w++) slot[2 + w] = k[w];
    slot[1] = meta;
    at = p;
    break;
  }
  *probe = probe_len(dist);
  return at;
}

// the wave's maximum of v into *dst (every lane of the wave calls)
__device__ inline void wave_max_to(u64* dst, uint32_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, (u64)v);
}
// the wave's count of `flag` added to *dst (every lane of the wave calls)
__device__ inline void wave_count_to(u64* dst, bool flag, bool negative = false) {
  const u64 m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) {
    const u64 c = (u64)__popcll(m);
    atomicAdd(dst, negative ? (u64)0 - c : c);
  }
}

// Exclusive prefix of v over the workgroup and the workgroup's total (every lane calls).
__device__ inline uint64_t wg_excl(uint64_t v, uint64_t* total) {
  __shared__ uint64_t wsum[WG / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  uint64_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)inc, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), d);
    if (lane >= (uint32_t)d) inc += ((uint64_t)hi << 32) | lo;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (uint32_t w = 0; w < WG / 64; w++) {
    if (w < wave) base += wsum[w];
    tot += wsum[w];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

constexpr uint32_t DG_NONE = mvk::DG_NONE;
constexpr uint32_t DG_MAX_AUTH = mvk::DG_MAX_AUTH;
constexpr int DG_BM = mvk::DG_BM_WORDS;
constexpr uint32_t DG_CAND = MV_DECIDE_MAX_LEADER_BLOCKS;

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ inline uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t wave_sum64(uint64_t v) {
  for (int d = 32; d; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
// the stake of the authorities of a 16-word bitmap (every lane of the wave calls; lane j sums j, j + 64, ...)
template <typename P>
__device__ inline uint64_t bitmap_stake(P bm, const uint64_t* __restrict__ stakes, uint32_t n_auth) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t stake = 0;
#pragma unroll
  for (uint32_t q = 0; q < DG_MAX_AUTH / 64; q++) {
    const uint32_t a = lane + 64 * q;
    if (a < n_auth && ((bm[a >> 5] >> (a & 31)) & 1u)) stake += stakes[a];
  }
  return wave_sum64(stake);
}

// the last of the n candidates whose first include (inc_base[], ascending from 0) is <= j
__device__ inline uint64_t cand_of_include(const uint64_t* __restrict__ inc_base, uint64_t n, uint64_t j) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (inc_base[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

static inline uint32_t grid_of(uint64_t items) { return (uint32_t)((items + WG - 1) / WG); }

// ---------------------------------------------------------------- the compaction pass (contract: above)
template <class F>
__global__ void __launch_bounds__(WG) k_compact_count(const F f, const mvk::WgScan w) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t a = 0, b = 0, tot;
  if constexpr (F::WEIGHTS == 2) f.weigh(i, &a, &b);
  else f.weigh(i, &a);
  (void)wg_excl(a, &tot);
  if (threadIdx.x == 0) w.count_a[blockIdx.x] = tot;
  if constexpr (F::WEIGHTS == 2) {
    (void)wg_excl(b, &tot);
    if (threadIdx.x == 0) w.count_b[blockIdx.x] = tot;
  }
}
template <class F>
__global__ void __launch_bounds__(WG) k_compact_list(const F f, const mvk::WgScan w) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t a = 0, b = 0, tot;
  if constexpr (F::WEIGHTS == 2) f.weigh(i, &a, &b);
  else f.weigh(i, &a);
  const uint64_t ra = w.base_a[blockIdx.x] + wg_excl(a, &tot);
  if constexpr (F::WEIGHTS == 2) {
    const uint64_t rb = w.base_b[blockIdx.x] + wg_excl(b, &tot);
    f.place(i, a, ra, b, rb);
  } else {
    f.place(i, a, ra);
  }
}
// count and scan(s) over n items (n > 0): *total_a (and *total_b) = the weights' sums; with `running`
// (may be null) the first weight's ranks stand behind *running, which grows by its total
template <class F>
static inline void compact_count(const F& f, uint64_t n, const mvk::WgScan& w, uint64_t* total_a, uint64_t* total_b,
                                 uint64_t* running, hipStream_t s) {
  const uint64_t nwg = mvk::index_groups(n);
  hipLaunchKernelGGL(k_compact_count<F>, dim3(grid_of(n)), dim3(WG), 0, s, f, w);
  (void)mvk::launch_index_scan(w.count_a, nwg, w.base_a, total_a, running, s);
  if constexpr (F::WEIGHTS == 2) (void)mvk::launch_index_scan(w.count_b, nwg, w.base_b, total_b, nullptr, s);
}
// count, scan(s), list; list = false (a cap of 0) only counts
template <class F>
static inline void compact_pass(const F& f, uint64_t n, const mvk::WgScan& w, uint64_t* total_a, uint64_t* total_b,
                                uint64_t* running, hipStream_t s, bool list = true) {
  compact_count(f, n, w, total_a, total_b, running, s);
  if (list) hipLaunchKernelGGL(k_compact_list<F>, dim3(grid_of(n)), dim3(WG), 0, s, f, w);
}

}  // namespace mv::ix
