// The device-resident index of block references (include/mysti_verify.h: mv_index_*,
// mv_accept_blocks, mv_connect_blocks): a set of BlockReferences with a state each -- MV_REF_HAVE,
// what BlockManager::exists_or_pending answers (block_manager.rs:142-144), MV_REF_STORED, what
// BlockStore::block_exists answers, or MV_REF_WANTED, a key of
// block_references_waiting that is not pending (BlockManager::missing, :90-97) -- and the kernels
// of one accept call around the block pipeline (process_blocks' skip, net_sync.rs:325-336, and the
// include lookups of add_blocks, block_manager.rs:62-98). Where references lie in a block:
// block_ref.h.
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "block_ref.h"
#include "kernels.h"

namespace mv {
namespace ix {

using mvk::IndexKeys;
using mvk::IndexTable;
typedef unsigned long long u64;

constexpr int WG = 256;
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
__device__ inline uint32_t* meta_of(u64* slot) { return reinterpret_cast<uint32_t*>(slot + 1); }

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

// wgbase[g] = the counts of the workgroups before g; *total = all of them (k_replay_scan's shape)
__global__ void __launch_bounds__(1024) k_ix_scan(const uint64_t* __restrict__ wgcount, uint64_t nwg,
                                                  uint64_t* __restrict__ wgbase, uint64_t* __restrict__ total) {
  __shared__ uint64_t part[1024];
  const uint64_t per = (nwg + 1023) / 1024;
  const uint64_t lo = per * threadIdx.x < nwg ? per * threadIdx.x : nwg;
  const uint64_t hi = lo + per < nwg ? lo + per : nwg;
  uint64_t sum = 0;
  for (uint64_t g = lo; g < hi; g++) sum += wgcount[g];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t acc = part[threadIdx.x] - sum;
  for (uint64_t g = lo; g < hi; g++) {
    wgbase[g] = acc;
    acc += wgcount[g];
  }
  if (threadIdx.x == 1023) *total = part[1023];
}

// ---------------------------------------------------------------- insert rounds
__global__ void __launch_bounds__(WG) k_ix_claim(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                 uint32_t newstate, int round, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool act = i < n;
  if (act && round == 0) {
    act = has_src(ks, i);
    if (!act) item[i] = pack(0, 0, C_NONE);
  } else if (act) {
    act = code_of(item[i]) == C_RETRY;
  }
  uint32_t probe = 0;
  bool fail = false;
  if (act) {
    uint64_t k[6], start, tag;
    load_key(ks, i, k);
    hash_key(t, k, &start, &tag);
    uint64_t p = round ? ((item[i] & SLOT_MASK) + 1) & t.mask : start;
    uint64_t dist = (p - start) & t.mask;  // slots already passed in earlier rounds
    const uint32_t me = ~(uint32_t)i;
    u64 res = pack(0, 0, C_FAIL);
    for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
      u64* slot = t.slots + SLOT_WORDS * p;
      const u64 old = atomicCAS(slot, 0ull, (u64)tag);
      if (old == 0) {
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, 0, C_CLAIMED);
        break;
      }
      if (old != tag) continue;
      const uint32_t st = __hip_atomic_load(meta_of(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (st == 0) {  // claimed in this launch: its key is not there yet
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, 0, C_CLAIMED);
        break;
      }
      if (!key_eq(slot, k)) continue;
      if (st >= newstate) {
        res = pack(p, st, C_NOOP);
      } else {
        atomicMax(meta_of(slot) + 1, me);
        res = pack(p, st, C_FOUND);
      }
      break;
    }
    probe = (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull);
    fail = code_of(res) == C_FAIL;
    item[i] = res;
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

__global__ void __launch_bounds__(WG) k_ix_fill(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                uint32_t newstate, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool created = false, raised = false;
  if (i < n) {
    const u64 it = item[i], c = code_of(it);
    if (c == C_CLAIMED || c == C_FOUND) {
      const uint64_t p = it & SLOT_MASK;
      u64* slot = t.slots + SLOT_WORDS * p;
      uint32_t* meta = meta_of(slot);
      const bool owner = meta[1] == ~(uint32_t)i;  // (set by k_ix_claim's atomics, an earlier kernel)
      if (c == C_CLAIMED && owner) {
        uint64_t k[6];
        load_key(ks, i, k);
#pragma unroll
        for (int w = 0; w < 6; w++) slot[2 + w] = k[w];
        atomicMax(meta, newstate);
        created = true;
        item[i] = pack(p, 0, C_NEW) | FRESH;
      } else if (c == C_FOUND) {
        if (owner) {
          atomicMax(meta, newstate);
          raised = true;
          item[i] = pack(p, prior_of(it), C_RAISED) | FRESH;
        } else {
          item[i] = pack(p, prior_of(it), C_DUP);
        }
      }
    }
  }
  // raises: WANTED -> HAVE, and WANTED or HAVE -> STORED (the HAVE counter holds HAVE and STORED)
  if (newstate >= MV_REF_HAVE) {
    const uint32_t prior = i < n ? prior_of(item[i]) : 0;  // (0 for an entry created now)
    wave_count_to(ctl + mvk::IX_CTL_HAVE, created || (raised && prior < MV_REF_HAVE));
    wave_count_to(ctl + mvk::IX_CTL_WANTED, raised && prior == MV_REF_WANTED, true);
    if (newstate == MV_REF_STORED) wave_count_to(ctl + mvk::IX_CTL_STORED, created || raised);
  } else {
    wave_count_to(ctl + mvk::IX_CTL_WANTED, created);
  }
}

__global__ void __launch_bounds__(WG) k_ix_settle(IndexTable t, IndexKeys ks, uint64_t n, u64* __restrict__ item,
                                                  u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool retry = false;
  if (i < n) {
    const u64 it = item[i];
    const uint64_t p = it & SLOT_MASK;
    u64* slot = t.slots + SLOT_WORDS * p;
    if (code_of(it) == C_CLAIMED) {  // not the owner: the owner's key is there since k_ix_fill
      uint64_t k[6];
      load_key(ks, i, k);
      retry = !key_eq(slot, k);
      item[i] = pack(p, 0, retry ? C_RETRY : C_DUP);
    } else if (it & FRESH) {
      meta_of(slot)[1] = 0;
      item[i] = it & ~FRESH;
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_RETRY, retry);
}

// after the last round a call enqueued ahead: items still left over are given up (the error word)
__global__ void k_ix_giveup(u64* __restrict__ ctl) {
  if (threadIdx.x || blockIdx.x) return;
  if (ctl[mvk::IX_CTL_RETRY]) atomicAdd(ctl + mvk::IX_CTL_ERR, ctl[mvk::IX_CTL_RETRY]);
}

__global__ void __launch_bounds__(WG) k_ix_prior(const u64* __restrict__ item, uint64_t n, uint8_t* __restrict__ prior) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i < n) prior[i] = (uint8_t)prior_of(item[i]);
}

// Read-only probe: the state of key k, MV_REF_ABSENT without an entry. Nothing writes the table
// in a launch that calls it. *probe = slots examined.
__device__ inline uint32_t lookup(const IndexTable& t, const uint64_t k[6], uint32_t* probe, bool* fail) {
  uint64_t start, tag;
  hash_key(t, k, &start, &tag);
  uint64_t p = start, dist = 0;
  uint32_t st = MV_REF_ABSENT;
  bool ended = false;
  for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
    const u64* slot = t.slots + SLOT_WORDS * p;
    const u64 g = slot[0];
    if (g == 0) {
      ended = true;
      break;
    }
    if (g == tag && key_eq(slot, k)) {
      st = (uint32_t)slot[1];
      ended = true;
      break;
    }
  }
  *probe = (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull);
  *fail = !ended;
  return st;
}

__global__ void __launch_bounds__(WG) k_ix_lookup(IndexTable t, IndexKeys ks, uint64_t n, uint8_t* __restrict__ out,
                                                  u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < n) {
    uint32_t st = MV_REF_ABSENT;
    if (t.slots && has_src(ks, i)) {
      uint64_t k[6];
      load_key(ks, i, k);
      st = lookup(t, k, &probe, &fail);
    }
    out[i] = (uint8_t)st;
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// One lane per slot of the old table: its entry into the new one. The keys are distinct, so a
// lane claims the first empty slot and never compares (no key of this launch is read).
__global__ void __launch_bounds__(WG) k_ix_rebuild(const u64* __restrict__ old, uint64_t old_slots, IndexTable t,
                                                   u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < old_slots) {
    const u64* src = old + SLOT_WORDS * i;
    const uint32_t st = (uint32_t)src[1];
    if (src[0] != 0 && st != 0) {
      uint64_t k[6], start, tag;
#pragma unroll
      for (int w = 0; w < 6; w++) k[w] = src[2 + w];
      hash_key(t, k, &start, &tag);
      uint64_t p = start, dist = 0;
      fail = true;
      for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
        u64* slot = t.slots + SLOT_WORDS * p;
        if (atomicCAS(slot, 0ull, (u64)tag) != 0) continue;
#pragma unroll
        for (int w = 0; w < 6; w++) slot[2 + w] = k[w];
        slot[1] = st;
        fail = false;
        break;
      }
      probe = (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull);
    }
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// The WANTED entries, listed by count / scan / list over the slots
__device__ inline bool slot_wanted(const u64* slots, uint64_t i, uint64_t n) {
  return i < n && slots[SLOT_WORDS * i] != 0 && (uint32_t)slots[SLOT_WORDS * i + 1] == MV_REF_WANTED;
}
__global__ void __launch_bounds__(WG) k_ix_wanted_count(const u64* __restrict__ slots, uint64_t n,
                                                        uint64_t* __restrict__ wgcount) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(slot_wanted(slots, i, n), &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(WG) k_ix_wanted_list(const u64* __restrict__ slots, uint64_t n,
                                                       const uint64_t* __restrict__ wgbase, uint64_t* __restrict__ out,
                                                       uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool w = slot_wanted(slots, i, n);
  uint64_t tot;
  const uint64_t r = wgbase[blockIdx.x] + wg_excl(w, &tot);
  if (!w || r >= cap) return;
#pragma unroll
  for (int k = 0; k < 6; k++) out[6 * r + k] = slots[SLOT_WORDS * i + 2 + k];
}

// ---------------------------------------------------------------- the accept call
using mvk::AcceptArrays;

__device__ inline bool block_inside(const AcceptArrays& a, uint64_t i) {
  return a.off[i] <= a.buf_bytes && a.len[i] <= a.buf_bytes - a.off[i];
}

// KNOWN: the block's own reference is HAVE or STORED in the index as it stands (net_sync.rs:325-336);
// counts the blocks that go on to verify per workgroup
__global__ void __launch_bounds__(WG) k_acc_probe(IndexTable t, AcceptArrays a, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false, known = false;
  if (i < a.n) {
    const uint64_t len = a.len[i];
    if (t.slots && block_inside(a, i) && br::own_ref_readable(len)) {
      const uint8_t* p = a.buf + a.off[i];
      if (ld64(p + br::LEN_WORD_OFF) == br::DIGEST_LEN) {
        uint64_t k[6];
#pragma unroll
        for (int w = 0; w < 6; w++) k[w] = ld64(p + br::key_word_off(w));
        known = lookup(t, k, &probe, &fail) >= MV_REF_HAVE;
      }
    }
    a.known[i] = known;
  }
  uint64_t tot;
  (void)wg_excl(i < a.n && !known, &tot);
  if (threadIdx.x == 0) a.wg_a[blockIdx.x] = tot;
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// the blocks to verify, in order
__global__ void __launch_bounds__(WG) k_acc_vlist(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool v = i < a.n && !a.known[i];
  uint64_t tot;
  const uint64_t r = a.base_a[blockIdx.x] + wg_excl(v, &tot);
  if (!v) return;
  a.v_off[r] = a.off[i];
  a.v_len[r] = a.len[i];
  a.rank[i] = (uint32_t)r;
}

__device__ inline bool group_head(const AcceptArrays& a, uint64_t i) {
  return i < a.n && (i == 0 || a.grp[i] != a.grp[i - 1]);
}
__global__ void __launch_bounds__(WG) k_acc_heads(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(group_head(a, i), &tot);
  if (threadIdx.x == 0) a.wg_a[blockIdx.x] = tot;
}

// statuses (KNOWN blocks are MV_BLOCK_OK unverified), the group of every block, and a reject flag
// per group: one rejected block drops its message before add_blocks (net_sync.rs:352-361)
__global__ void __launch_bounds__(WG) k_acc_groups(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t g = i;
  if (a.grp) {
    const bool head = group_head(a, i);
    uint64_t tot;
    g = a.base_a[blockIdx.x] + wg_excl(head, &tot) + head - 1;  // heads up to and including i, less one
  }
  if (i >= a.n) return;
  const bool known = a.known[i];
  const uint8_t st = known ? (uint8_t)MV_BLOCK_OK : a.v_status[a.rank[i]];
  a.status[i] = st;
  a.gidx[i] = (uint32_t)g;
  if (!known && st != MV_BLOCK_OK) atomicMax(a.gflag + g, 1u);
}

// states before the duplicates are told apart (candidates are MV_ACC_NEW for now), the include
// count of every candidate, and the per-workgroup counts of both
__global__ void __launch_bounds__(WG) k_acc_states(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool cand = false;
  uint64_t k = 0;
  if (i < a.n) {
    uint8_t s;
    if (a.known[i]) s = MV_ACC_KNOWN;
    else if (a.status[i] != MV_BLOCK_OK) s = MV_ACC_REJECTED;
    else if (a.gflag[a.gidx[i]]) s = MV_ACC_DROPPED;
    else s = MV_ACC_NEW, cand = true;
    // (a block that parsed holds its own reference and its includes; checked again all the same)
    const uint64_t len = a.len[i];
    if (cand && !(block_inside(a, i) && br::own_ref_readable(len))) s = MV_ACC_REJECTED, cand = false;
    if (cand && br::inc_count_readable(len)) {
      k = ld64(a.buf + a.off[i] + br::INC_COUNT_OFF);
      if (!br::includes_inside(len, k)) k = 0;
    }
    a.state[i] = s;
    a.kc[i] = (uint32_t)k;
  }
  uint64_t tc, tk;
  (void)wg_excl(cand, &tc);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    a.wg_a[blockIdx.x] = tc;
    a.wg_b[blockIdx.x] = tk;
  }
}

// the candidates in block order: block, where its own reference lies, its first include's number
__global__ void __launch_bounds__(WG) k_acc_cand_list(AcceptArrays a) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool cand = i < a.n && a.state[i] == MV_ACC_NEW;
  const uint64_t k = cand ? a.kc[i] : 0;
  uint64_t tc, tk;
  const uint64_t r = a.base_a[blockIdx.x] + wg_excl(cand, &tc);
  const uint64_t ib = a.base_b[blockIdx.x] + wg_excl(k, &tk);
  if (!cand) return;
  a.cand_blk[r] = (uint32_t)i;
  a.cand_src[r] = a.off[i];
  a.inc_base[r] = ib;
}

// the lowest block of every reference is NEW, the others DUP (block_manager.rs:68-72)
__global__ void __launch_bounds__(WG) k_acc_own_states(AcceptArrays a, const u64* __restrict__ item, uint64_t ncand) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (r >= ncand) return;
  const u64 c = code_of(item[r]);
  a.state[a.cand_blk[r]] = (c == C_NEW || c == C_RAISED) ? MV_ACC_NEW : MV_ACC_DUP;
}

// one lane per include of the candidates: where it lies, or IX_NO_SRC when its block is not NEW
__global__ void __launch_bounds__(WG) k_acc_inc_src(AcceptArrays a, uint64_t ncand, uint64_t ninc,
                                                    uint64_t* __restrict__ inc_src) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= ninc) return;
  uint64_t lo = 0, hi = ncand;  // the last candidate whose first include is <= j
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.inc_base[mid] <= j) lo = mid;
    else hi = mid;
  }
  const uint64_t q = j - a.inc_base[lo];
  const bool is_new = a.state[a.cand_blk[lo]] == MV_ACC_NEW && q < a.kc[a.cand_blk[lo]];
  inc_src[j] = is_new ? a.cand_src[lo] + br::include_off(q) : mvk::IX_NO_SRC;
}

// the includes that created an entry are the missing references, in (block, include) order
__global__ void __launch_bounds__(WG) k_acc_miss_count(const u64* __restrict__ item, uint64_t n,
                                                       uint64_t* __restrict__ wgcount) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(j < n && code_of(item[j]) == C_NEW, &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(WG) k_acc_miss_list(IndexTable t, const u64* __restrict__ item, uint64_t n,
                                                      const uint64_t* __restrict__ wgbase, uint64_t* __restrict__ out,
                                                      uint64_t cap) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool m = j < n && code_of(item[j]) == C_NEW;
  uint64_t tot;
  const uint64_t r = wgbase[blockIdx.x] + wg_excl(m, &tot);
  if (!m || r >= cap) return;
  const u64* slot = t.slots + SLOT_WORDS * (item[j] & SLOT_MASK);
#pragma unroll
  for (int k = 0; k < 6; k++) out[6 * r + k] = slot[2 + k];
}

// ---------------------------------------------------------------- the suspended-block store and the connect sweep
// mv_connect_blocks: the suspend / unlock cascade of add_blocks (block_manager.rs:102-131) as a
// least fixed point -- a suspended block is stored exactly when all its includes are stored. A
// record holds slots of the table, not keys: a level's check is one 8-byte load per include, and
// the reference words of a row are read from the block's own slot. Level l is four launches on
// one stream:
//   k_pb_check   a wave per record not connected yet: every include's state is STORED (and its
//                own is not). It reads only states raised by earlier launches.
//   k_pb_count, k_pb_scan   the hits per workgroup and their places behind the rows so far
//   k_pb_list    a hit writes its row (below the cap), notes its level and raises its own state
//                by atomicMax. Nothing in this launch reads a state.
// Within a level the scan orders rows by record, which is arrival order: compaction is stable
// and appends go in block order. No lane waits for another; the host enqueues levels until one
// lists nothing, at most records + 1 of them.
using mvk::PendStore;

__device__ inline uint32_t slot_state(const u64* slots, uint64_t p) { return (uint32_t)slots[SLOT_WORDS * p + 1]; }

__global__ void __launch_bounds__(WG) k_pb_own_slots(const u64* __restrict__ item, uint64_t ncand,
                                                     uint64_t* __restrict__ cand_slot) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (r < ncand) cand_slot[r] = item[r] & SLOT_MASK;
}

// the NEW blocks among the candidates and their includes, per workgroup
__global__ void __launch_bounds__(WG) k_pb_app_count(AcceptArrays a, uint64_t ncand, uint64_t* __restrict__ wg_a,
                                                     uint64_t* __restrict__ wg_b) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool nw = r < ncand && a.state[a.cand_blk[r]] == MV_ACC_NEW;
  const uint64_t k = nw ? a.kc[a.cand_blk[r]] : 0;
  uint64_t tb, tk;
  (void)wg_excl(nw, &tb);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}
__global__ void __launch_bounds__(WG) k_pb_app_list(AcceptArrays a, uint64_t ncand, const uint64_t* __restrict__ cand_slot,
                                                    const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b,
                                                    PendStore p, uint64_t nb0, uint64_t ni0, uint64_t* __restrict__ cand_dst) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool nw = r < ncand && a.state[a.cand_blk[r]] == MV_ACC_NEW;
  const uint64_t k = nw ? a.kc[a.cand_blk[r]] : 0;
  uint64_t tb, tk;
  const uint64_t rb = nb0 + base_a[blockIdx.x] + wg_excl(nw, &tb);
  const uint64_t ib = ni0 + base_b[blockIdx.x] + wg_excl(k, &tk);
  if (r >= ncand) return;
  cand_dst[r] = nw ? ib : mvk::IX_NO_SRC;
  if (!nw) return;
  p.slot[rb] = cand_slot[r];
  p.ibase[rb] = ib;
  p.blk[rb] = a.cand_blk[r];
  p.kc[rb] = (uint32_t)k;
}
// one lane per include of the candidates (k_acc_inc_src's shape): its slot into its block's record
__global__ void __launch_bounds__(WG) k_pb_app_inc(AcceptArrays a, uint64_t ncand, uint64_t ninc, const u64* __restrict__ item,
                                                   const uint64_t* __restrict__ cand_dst, PendStore p) {
  const uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (j >= ninc) return;
  uint64_t lo = 0, hi = ncand;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a.inc_base[mid] <= j) lo = mid;
    else hi = mid;
  }
  const uint64_t q = j - a.inc_base[lo];
  if (cand_dst[lo] != mvk::IX_NO_SRC && q < a.kc[a.cand_blk[lo]]) p.inc[cand_dst[lo] + q] = item[j] & SLOT_MASK;
}

__global__ void __launch_bounds__(WG) k_pb_check(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                 const uint32_t* __restrict__ lvl, uint8_t* __restrict__ hit) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // the same for the whole wave
  const uint32_t lane = threadIdx.x & 63;
  if (b >= nb) return;
  bool ok = lvl[b] == 0 && slot_state(slots, p.slot[b]) != MV_REF_STORED;
  if (ok) {
    const uint64_t base = p.ibase[b];
    const uint32_t kc = p.kc[b];
    for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave leaves together
      const uint32_t q = q0 + lane;
      const bool bad = q < kc && slot_state(slots, p.inc[base + q]) != MV_REF_STORED;
      if (__ballot(bad)) {
        ok = false;
        break;
      }
    }
  }
  if (lane == 0) hit[b] = ok;
}
__global__ void __launch_bounds__(WG) k_pb_count(const uint8_t* __restrict__ hit, uint64_t nb, uint64_t* __restrict__ wgcount) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(b < nb && hit[b], &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
// k_ix_scan behind the rows listed so far: wgbase[g] = *rows + the counts before g; *level_rows =
// this level's; *rows += them
__global__ void __launch_bounds__(1024) k_pb_scan(const uint64_t* __restrict__ wgcount, uint64_t nwg,
                                                  uint64_t* __restrict__ wgbase, uint64_t* __restrict__ rows,
                                                  uint64_t* __restrict__ level_rows) {
  __shared__ uint64_t part[1024];
  const uint64_t before = *rows;  // (written below by one lane, after every barrier)
  const uint64_t per = (nwg + 1023) / 1024;
  const uint64_t lo = per * threadIdx.x < nwg ? per * threadIdx.x : nwg;
  const uint64_t hi = lo + per < nwg ? lo + per : nwg;
  uint64_t sum = 0;
  for (uint64_t g = lo; g < hi; g++) sum += wgcount[g];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t acc = before + part[threadIdx.x] - sum;
  for (uint64_t g = lo; g < hi; g++) {
    wgbase[g] = acc;
    acc += wgcount[g];
  }
  if (threadIdx.x == 1023) {
    *level_rows = part[1023];
    *rows = before + part[1023];
  }
}
__global__ void __launch_bounds__(WG) k_pb_list(u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                const uint8_t* __restrict__ hit, const uint64_t* __restrict__ wgbase,
                                                uint32_t* __restrict__ lvl, uint64_t level, uint64_t* __restrict__ out,
                                                uint64_t cap, u64* __restrict__ ctl, uint32_t* __restrict__ row_of) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool h = b < nb && hit[b];
  uint64_t tot;
  const uint64_t r = wgbase[blockIdx.x] + wg_excl(h, &tot);
  if (h) {
    u64* slot = slots + SLOT_WORDS * p.slot[b];
    lvl[b] = (uint32_t)level + 1;
    if (row_of) row_of[b] = (uint32_t)r;  // (with a DAG store: its record order is the row order)
    if (r < cap) {
#pragma unroll
      for (int w = 0; w < 6; w++) out[8 * r + w] = slot[2 + w];  // (the key: written by an earlier launch)
      out[8 * r + 6] = p.blk[b];
      out[8 * r + 7] = level;
    }
    atomicMax(meta_of(slot), (uint32_t)MV_REF_STORED);
  }
  wave_count_to(ctl + mvk::IX_CTL_STORED, h);
}

// compaction: the records whose own reference is not STORED stay, in order
__global__ void __launch_bounds__(WG) k_pb_keep_count(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                      uint64_t* __restrict__ wg_a, uint64_t* __restrict__ wg_b) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool keep = b < nb && slot_state(slots, p.slot[b]) != MV_REF_STORED;
  uint64_t tb, tk;
  (void)wg_excl(keep, &tb);
  (void)wg_excl(keep ? p.kc[b] : 0, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}
__global__ void __launch_bounds__(WG) k_pb_keep_list(const u64* __restrict__ slots, PendStore p, PendStore q, uint64_t nb,
                                                     const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b,
                                                     uint64_t* __restrict__ newbase, uint8_t* __restrict__ state,
                                                     uint64_t n_state) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool keep = b < nb && slot_state(slots, p.slot[b]) != MV_REF_STORED;
  uint64_t tb, tk;
  const uint64_t rb = base_a[blockIdx.x] + wg_excl(keep, &tb);
  const uint64_t ib = base_b[blockIdx.x] + wg_excl(keep ? p.kc[b] : 0, &tk);
  if (b >= nb) return;
  newbase[b] = keep ? ib : mvk::IX_NO_SRC;
  if (!keep) return;
  q.slot[rb] = p.slot[b];
  q.ibase[rb] = ib;
  q.blk[rb] = mvk::IX_NO_SRC;  // the next call finds it suspended by an earlier one
  q.kc[rb] = p.kc[b];
  if (p.blk[b] < n_state) state[p.blk[b]] = MV_ACC_SUSPENDED;  // (n_state is 0 without a state array)
}
__global__ void __launch_bounds__(WG) k_pb_keep_inc(PendStore p, PendStore q, uint64_t nb, const uint64_t* __restrict__ newbase) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (b >= nb || newbase[b] == mvk::IX_NO_SRC) return;
  const uint64_t from = p.ibase[b], to = newbase[b];
  const uint32_t kc = p.kc[b];
  for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) q.inc[to + i] = p.inc[from + i];
}

// after k_ix_rebuild: slot numbers of the old table become those of the same keys in the new one
// (read-only probes of a table that an earlier launch filled)
__global__ void __launch_bounds__(WG) k_pb_reresolve(const u64* __restrict__ old, IndexTable t, uint64_t* __restrict__ slotidx,
                                                     uint64_t n, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t probe = 0;
  bool fail = false;
  if (i < n) {
    const u64* src = old + SLOT_WORDS * slotidx[i];
    uint64_t k[6], start, tag;
#pragma unroll
    for (int w = 0; w < 6; w++) k[w] = src[2 + w];
    hash_key(t, k, &start, &tag);
    uint64_t p = start, dist = 0;
    fail = true;
    for (; dist <= t.mask; dist++, p = (p + 1) & t.mask) {
      const u64* slot = t.slots + SLOT_WORDS * p;
      const u64 g = slot[0];
      if (g == 0) break;
      if (g == tag && key_eq(slot, k)) {
        slotidx[i] = p;
        fail = false;
        break;
      }
    }
    probe = (uint32_t)(dist < 0xffffffffull ? dist + 1 : 0xffffffffull);
  }
  wave_max_to(ctl + mvk::IX_CTL_MAXPROBE, probe);
  wave_count_to(ctl + mvk::IX_CTL_ERR, fail);
}

// ---------------------------------------------------------------- the DAG store and the direct decision rule
// mv_dag_reserve / mv_decide_leaders: the edges of the blocks mv_connect_blocks stored, and
// BaseCommitter::try_direct_decide at wave length 3 over them (base_committer.rs:228-357; the
// wording of every predicate is the header's). A record holds slots of the table, as PendStore
// does; map[] gives the record of a slot. The memory model is the one at the top of this file:
// lanes of one launch talk only through agent-scope atomic read-modify-writes on single words
// (atomicOr into a bitmap, atomicAdd on a candidate count, atomicMax on a control word), no lane
// waits for another, and what a kernel reads as plain data an earlier launch wrote. Inside one
// wave, k_dg_cert collects a bitmap in LDS under wave-scope fences. Every slot number is checked
// against the table size and every record number against the store's count before it is an
// address; a number out of range counts into the error word (MV_E_HIP) and is not followed.
//   k_dg_app_*   a connect call's rows join the store: records (and map[]), the scan of their
//                include counts, the include slots a wave per row
//   k_dg_keep_*  mv_dag_prune: k_pb_keep_*'s shape over "round >= floor"
//   k_dg_pick_*  a lane per record: is it a voting (r + 1) or a decision (r + 2) record of a leader
//                round, by binary search over the sorted distinct rounds; count / scan / list into
//                vlist and dlist; a leader block adds itself to its rows' candidates
//   k_dg_vote    a wave per (voting record, row of that round): any include of the authority, the
//                first (authority, round) include in include order across batches of 64
//   k_dg_cert    a wave per (decision record, row): the vote authors among its includes per candidate
//   k_dg_decide  a wave per row: stakes of the bitmaps, the status and the row
using mvk::DagStore;
using mvk::DecideIn;
using mvk::DecideState;
constexpr uint32_t DG_NONE = mvk::DG_NONE;
constexpr u64 DG_NO_SLOT = mvk::DG_NO_SLOT;
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

__global__ void __launch_bounds__(WG) k_dg_app_rows(const u64* __restrict__ slots, PendStore p, uint64_t nb,
                                                    const uint32_t* __restrict__ lvl, const uint32_t* __restrict__ row_of,
                                                    uint64_t rows, DagStore d, uint64_t nb0, uint64_t* __restrict__ src,
                                                    u64* __restrict__ ctl) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (b < nb && lvl[b] != 0) {
    const uint64_t r = row_of[b], s = p.slot[b], rec = nb0 + r;
    bad = r >= rows || rec >= d.cap_b || s >= d.n_slots;
    if (!bad) {
      const u64* slot = slots + SLOT_WORDS * s;  // (the key: written by an earlier launch)
      const u64 a = slot[2], rd = slot[3];
      d.slot[rec] = s;
      d.auth[rec] = a < DG_MAX_AUTH ? (uint32_t)a : DG_NONE;
      d.round[rec] = rd;
      d.kc[rec] = p.kc[b];
      d.map[s] = (uint32_t)rec;
      src[r] = b;
      atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
      atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}
// (src[r] is IX_NO_SRC for a row k_dg_app_rows refused: its record is not read)
__device__ inline uint64_t app_kc(const DagStore& d, uint64_t nb0, uint64_t rows, const uint64_t* src, uint64_t r) {
  return r < rows && src[r] != mvk::IX_NO_SRC ? d.kc[nb0 + r] : 0;
}
__global__ void __launch_bounds__(WG) k_dg_app_count(DagStore d, uint64_t nb0, uint64_t rows, const uint64_t* __restrict__ src,
                                                     uint64_t* __restrict__ wgcount) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(app_kc(d, nb0, rows, src, r), &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(WG) k_dg_app_list(DagStore d, uint64_t nb0, uint64_t ni0, uint64_t rows,
                                                    const uint64_t* __restrict__ src, const uint64_t* __restrict__ wgbase) {
  const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  const uint64_t ib = ni0 + wgbase[blockIdx.x] + wg_excl(app_kc(d, nb0, rows, src, r), &tot);
  if (r < rows && src[r] != mvk::IX_NO_SRC) d.ibase[nb0 + r] = ib;
}
__global__ void __launch_bounds__(WG) k_dg_app_inc(PendStore p, uint64_t nb, DagStore d, uint64_t nb0, uint64_t rows,
                                                   const uint64_t* __restrict__ src, u64* __restrict__ ctl) {
  const uint64_t r = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  if (r >= rows) return;
  const uint64_t b = src[r];
  bool bad = b >= nb;
  if (!bad) {
    const uint64_t from = p.ibase[b], to = d.ibase[nb0 + r];
    const uint32_t kc = d.kc[nb0 + r];
    bad = to > d.cap_i || kc > d.cap_i - to;
    if (!bad)
      for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) d.inc[to + i] = p.inc[from + i];
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && (threadIdx.x & 63) == 0);
}

__global__ void __launch_bounds__(WG) k_dg_map(DagStore d, uint64_t nb, u64* __restrict__ ctl) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (b < nb) {
    const uint64_t s = d.slot[b];
    bad = s >= d.n_slots;
    if (!bad) d.map[s] = (uint32_t)b;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_dg_keep_count(DagStore d, uint64_t nb, uint64_t floor, uint64_t* __restrict__ wg_a,
                                                      uint64_t* __restrict__ wg_b) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool keep = b < nb && d.round[b] >= floor;
  uint64_t tb, tk;
  (void)wg_excl(keep, &tb);
  (void)wg_excl(keep ? d.kc[b] : 0, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}
__global__ void __launch_bounds__(WG) k_dg_keep_list(DagStore d, DagStore q, uint64_t nb, uint64_t floor,
                                                     const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b,
                                                     uint64_t* __restrict__ newbase, u64* __restrict__ ctl) {
  const uint64_t b = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool keep = b < nb && d.round[b] >= floor;
  const uint32_t kc = keep ? d.kc[b] : 0;
  uint64_t tb, tk;
  const uint64_t rb = base_a[blockIdx.x] + wg_excl(keep, &tb);
  const uint64_t ib = base_b[blockIdx.x] + wg_excl(kc, &tk);
  bool bad = false;
  if (b < nb) {
    const uint64_t s = keep ? d.slot[b] : 0;
    bad = keep && (rb >= q.cap_b || ib > q.cap_i || kc > q.cap_i - ib || s >= q.n_slots);
    keep = keep && !bad;
    newbase[b] = keep ? ib : mvk::IX_NO_SRC;
    if (keep) {
      const uint64_t rd = d.round[b];
      q.slot[rb] = s;
      q.auth[rb] = d.auth[b];
      q.round[rb] = rd;
      q.ibase[rb] = ib;
      q.kc[rb] = kc;
      q.map[s] = (uint32_t)rb;
      atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
      atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}
__global__ void __launch_bounds__(WG) k_dg_keep_inc(DagStore d, DagStore q, uint64_t nb, const uint64_t* __restrict__ newbase) {
  const uint64_t b = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (b >= nb || newbase[b] == mvk::IX_NO_SRC) return;
  const uint64_t from = d.ibase[b], to = newbase[b];
  const uint32_t kc = d.kc[b];
  if (from > d.cap_i || kc > d.cap_i - from) return;  // (k_dg_keep_list checked the other side)
  for (uint32_t i = threadIdx.x & 63; i < kc; i += 64) q.inc[to + i] = d.inc[from + i];
}

// ---------------------------------------------------------------- seeding the DAG store from a replay's rows
// mv_dev_dag_seed_rows / mv_wal_recover: the rows of mv_wal_replay become stored blocks with records
// (BlockStore::open with add_unloaded, block_store.rs:50-116, 398-404; the wording of every rule is
// the header's). The blocks are read in place in the image; a row's offset and length are the
// caller's, so they are checked against the image before a byte is read, and the include count
// against the length before it counts. Between the kernels stand the two inserts of the call (the
// rows' own references towards STORED, the record rows' includes towards WANTED), both by
// k_ix_claim / fill / settle. The memory model is the one at the top of this file:
//   k_sd_elig     a lane per row: may it get a record (OK, round >= floor, its bytes fit), its include
//                 count; the eligible rows and their includes per workgroup (they decide about room)
//   k_sd_claim    after the own references' insert: a row's slot, and atomicMin of nb0 + row into
//                 map[slot] -- a record from before the call is below nb0 and stays, otherwise the
//                 lowest row of a reference wins, as the lowest item owns a slot in k_ix_claim
//   k_sd_count    first[row] = map[slot] == nb0 + row (what k_sd_claim left), the record rows and
//                 their includes per workgroup
//   k_sd_list     a record row writes its record, map[slot] and where its block lies; a first row
//                 without a record puts map[slot] back to DG_NONE. It reads first[], not map[].
//   k_sd_inc_src  a wave per record: where its includes lie in the image, for the includes' insert
//   k_sd_inc      a wave per record: the slots that insert found, in batches of 64
using mvk::SeedRows;
constexpr uint8_t SD_ELIGIBLE = 1, SD_MISFIT = 2;

__global__ void __launch_bounds__(WG) k_sd_elig(SeedRows r, uint64_t* __restrict__ wg_a, uint64_t* __restrict__ wg_b,
                                                u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool el = false, misfit = false;
  uint64_t k = 0;
  if (i < r.n) {
    const uint64_t* row = r.rows + mvk::SD_ROW_WORDS * i;
    if (r.status[i] == MV_BLOCK_OK) {
      const uint64_t off = row[1], len = row[2];
      bool fits = off <= r.size && len <= r.size - off && br::inc_count_readable(len);
      if (fits) {
        k = ld64(r.img + off + br::INC_COUNT_OFF);
        fits = br::includes_inside(len, k) && k <= 0xffffffffull;
      }
      misfit = !fits;
      el = fits && row[4] >= r.floor;
    }
    if (!el) k = 0;
    r.elig[i] = el ? SD_ELIGIBLE : misfit ? SD_MISFIT : 0;
    r.kc[i] = (uint32_t)k;
  }
  uint64_t te, tk;
  (void)wg_excl(el, &te);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = te;
    wg_b[blockIdx.x] = tk;
  }
  wave_count_to(ctl + mvk::IX_CTL_SD_MISFIT, misfit);
}

__device__ inline bool item_has_slot(u64 it) {
  const u64 c = code_of(it);
  return c == C_NEW || c == C_RAISED || c == C_DUP || c == C_NOOP;
}

__global__ void __launch_bounds__(WG) k_sd_claim(const u64* __restrict__ item, SeedRows r, DagStore d, uint64_t nb0,
                                                 u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (i < r.n) {
    const u64 it = item[i];
    const uint64_t s = it & SLOT_MASK;
    bad = !item_has_slot(it) || s >= d.n_slots;
    r.own_slot[i] = bad ? mvk::IX_NO_SRC : s;
    if (!bad) atomicMin(d.map + s, (uint32_t)(nb0 + i));
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_sd_count(SeedRows r, DagStore d, uint64_t nb0, uint64_t* __restrict__ wg_a,
                                                 uint64_t* __restrict__ wg_b) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool rec = false;
  uint64_t k = 0;
  if (i < r.n) {
    const uint64_t s = r.own_slot[i];
    const bool first = s < d.n_slots && d.map[s] == (uint32_t)(nb0 + i);  // (k_sd_claim's atomics, an earlier kernel)
    r.first[i] = first;
    rec = first && r.elig[i] == SD_ELIGIBLE;
    k = rec ? r.kc[i] : 0;
  }
  uint64_t tb, tk;
  (void)wg_excl(rec, &tb);
  (void)wg_excl(k, &tk);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tb;
    wg_b[blockIdx.x] = tk;
  }
}

__global__ void __launch_bounds__(WG) k_sd_list(const u64* __restrict__ slots, SeedRows r, DagStore d, uint64_t nb0,
                                                uint64_t ni0, const uint64_t* __restrict__ base_a,
                                                const uint64_t* __restrict__ base_b, u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool first = i < r.n && r.first[i];
  const bool rec = first && r.elig[i] == SD_ELIGIBLE;
  const uint64_t k = rec ? r.kc[i] : 0;
  uint64_t tb, tk;
  const uint64_t rb = nb0 + base_a[blockIdx.x] + wg_excl(rec, &tb);
  const uint64_t ib = ni0 + base_b[blockIdx.x] + wg_excl(k, &tk);
  bool bad = false;
  if (first) {
    const uint64_t s = r.own_slot[i];  // (below the table's size: k_sd_count checked it)
    bad = rec && (rb >= d.cap_b || rb - nb0 >= r.n || ib > d.cap_i || k > d.cap_i - ib);
    if (rec && !bad) {
      const u64* slot = slots + SLOT_WORDS * s;  // (the key: written by an earlier launch)
      const u64 a = slot[2], rd = slot[3];
      d.slot[rb] = s;
      d.auth[rb] = a < DG_MAX_AUTH ? (uint32_t)a : DG_NONE;
      d.round[rb] = rd;
      d.kc[rb] = (uint32_t)k;
      d.ibase[rb] = ib;
      d.map[s] = (uint32_t)rb;
      r.rec_off[rb - nb0] = r.rows[mvk::SD_ROW_WORDS * i + 1];
      atomicMax(ctl + mvk::IX_CTL_DG_NLO, ~rd);
      atomicMax(ctl + mvk::IX_CTL_DG_HI, rd);
    } else {
      d.map[s] = DG_NONE;  // the claim of a row that gets no record
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// where the includes of the call's record `rec` stand among the call's include items; false: out of range
__device__ inline bool seed_span(const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t ninc, uint64_t rec, uint64_t* base,
                                 uint32_t* kc) {
  const uint64_t ib = d.ibase[nb0 + rec];
  *kc = d.kc[nb0 + rec];
  *base = ib - ni0;
  return ib >= ni0 && ib - ni0 <= ninc && *kc <= ninc - (ib - ni0) && ib <= d.cap_i && *kc <= d.cap_i - ib;
}
__global__ void __launch_bounds__(WG) k_sd_inc_src(SeedRows r, DagStore d, uint64_t nb0, uint64_t ni0, uint64_t nrec,
                                                   uint64_t ninc, uint64_t* __restrict__ inc_src, u64* __restrict__ ctl) {
  const uint64_t rec = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (rec >= nrec) return;
  uint64_t base;
  uint32_t kc;
  const bool bad = !seed_span(d, nb0, ni0, ninc, rec, &base, &kc);
  if (!bad) {
    const uint64_t off = r.rec_off[rec];  // (k_sd_elig checked off + 64 + 56 kc against the image)
    for (uint32_t q = threadIdx.x & 63; q < kc; q += 64) inc_src[base + q] = off + br::include_off(q);
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && (threadIdx.x & 63) == 0);
}
__global__ void __launch_bounds__(WG) k_sd_inc(const u64* __restrict__ item, DagStore d, uint64_t nb0, uint64_t ni0,
                                               uint64_t nrec, uint64_t ninc, u64* __restrict__ ctl) {
  const uint64_t rec = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record
  if (rec >= nrec) return;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t base;
  uint32_t kc;
  bool bad = !seed_span(d, nb0, ni0, ninc, rec, &base, &kc);
  uint64_t nbad = bad && lane == 0;
  if (!bad) {
    for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
      const uint32_t q = q0 + lane;
      if (q >= kc) continue;
      const u64 it = item[base + q];
      const uint64_t s = it & SLOT_MASK;
      const bool ok = item_has_slot(it) && s < d.n_slots;
      d.inc[ni0 + base + q] = ok ? s : DG_NO_SLOT;
      nbad += !ok;
    }
  }
  nbad = wave_sum64(nbad);
  if (lane == 0 && nbad) atomicAdd(ctl + mvk::IX_CTL_ERR, (u64)nbad);
}

// *g = the place of `round` among the call's distinct leader rounds
__device__ inline bool leader_group(const DecideIn& in, uint64_t round, uint64_t* g) {
  uint64_t lo = 0, hi = in.ng;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (in.g_round[mid] < round) lo = mid + 1;
    else hi = mid;
  }
  *g = lo;
  return lo < in.ng && in.g_round[lo] == round;
}
__device__ inline void pick_roles(const DagStore& d, uint64_t nb, const DecideIn& in, uint64_t rec, bool* voting,
                                  bool* decision) {
  uint64_t g;
  const uint64_t rd = rec < nb ? d.round[rec] : 0;
  *voting = rec < nb && rd >= 1 && leader_group(in, rd - 1, &g);
  *decision = rec < nb && rd >= 2 && leader_group(in, rd - 2, &g);
}
__global__ void __launch_bounds__(WG) k_dg_pick_count(DagStore d, uint64_t nb, DecideIn in, uint64_t* __restrict__ wg_a,
                                                      uint64_t* __restrict__ wg_b) {
  const uint64_t rec = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool v, c;
  pick_roles(d, nb, in, rec, &v, &c);
  uint64_t tv, tc;
  (void)wg_excl(v, &tv);
  (void)wg_excl(c, &tc);
  if (threadIdx.x == 0) {
    wg_a[blockIdx.x] = tv;
    wg_b[blockIdx.x] = tc;
  }
}
__global__ void __launch_bounds__(WG) k_dg_pick_list(DagStore d, uint64_t nb, DecideIn in, DecideState st,
                                                     const uint64_t* __restrict__ base_a, const uint64_t* __restrict__ base_b) {
  const uint64_t rec = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool v, c;
  pick_roles(d, nb, in, rec, &v, &c);
  uint64_t tv, tc;
  const uint64_t pv = base_a[blockIdx.x] + wg_excl(v, &tv);
  const uint64_t pc = base_b[blockIdx.x] + wg_excl(c, &tc);
  if (rec >= nb) return;
  st.vpos[rec] = v && pv < nb ? (uint32_t)pv : DG_NONE;
  if (v && pv < nb) st.vlist[pv] = (uint32_t)rec;
  if (c && pc < nb) st.dlist[pc] = (uint32_t)rec;
  uint64_t g;
  if (!leader_group(in, d.round[rec], &g)) return;
  // a leader block of every row (authority, round) that names it; bounded by the rows of the round
  const uint64_t a = d.auth[rec], hi = in.g_start[g + 1] < in.n ? in.g_start[g + 1] : in.n;
  for (uint64_t k = in.g_start[g]; k < hi; k++) {
    if (in.l_auth[k] != a) continue;
    const uint32_t at = atomicAdd(st.cand_n + k, 1u);
    if (at < DG_CAND) st.cand_slot[DG_CAND * k + at] = d.slot[rec];
  }
}

// which (record of a list, row) a wave works on; false: none
__device__ inline bool wave_task(const DagStore& d, uint64_t nb, const DecideIn& in, const uint32_t* __restrict__ list,
                                 uint64_t n_list, uint64_t back, uint64_t* at, uint64_t* j, uint64_t* rec, uint64_t* k,
                                 bool* bad) {
  const uint64_t w = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // the same for the whole wave
  *at = w / in.gmax, *j = w % in.gmax;
  if (*at >= n_list) return false;
  *rec = list[*at];
  if (*rec >= nb) {
    *bad = true;
    return false;
  }
  const uint64_t rd = d.round[*rec];
  uint64_t g;
  if (rd < back || !leader_group(in, rd - back, &g)) return false;
  *k = in.g_start[g] + *j;
  return *k < in.g_start[g + 1] && *k < in.n;
}

__global__ void __launch_bounds__(WG) k_dg_vote(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                DecideState st, uint64_t nvote, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t vi, j, rec, k;
  bool bad = false;
  if (wave_task(d, nb, in, st.vlist, nvote, 1, &vi, &j, &rec, &k, &bad)) {
    const uint64_t a = in.l_auth[k], r = in.l_round[k];
    const uint64_t base = d.ibase[rec];
    const uint32_t kc = d.kc[rec];
    bad = base > d.cap_i || kc > d.cap_i - base;
    if (!bad) {
      bool any = false;
      u64 sup = DG_NO_SLOT;
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
        const uint32_t q = q0 + lane;
        u64 s = DG_NO_SLOT;
        bool has_a = false, match = false;
        if (q < kc) {
          s = d.inc[base + q];
          if (s < d.n_slots) {
            has_a = slots[SLOT_WORDS * s + 2] == a;  // the authority only (base_committer.rs:234-237)
            match = has_a && slots[SLOT_WORDS * s + 3] == r;
          } else {
            bad = true;
          }
        }
        any = any || __ballot(has_a) != 0;
        const u64 m = __ballot(match);
        if (m && sup == DG_NO_SLOT) sup = shfl64(s, __ffsll((long long)m) - 1);  // the first in include order
      }
      const uint32_t author = d.auth[rec];
      if (lane == 0) {
        st.sup[vi * in.gmax + j] = sup;
        if (author < DG_MAX_AUTH) {
          const uint32_t bit = 1u << (author & 31);
          if (!any) atomicOr(st.blame + DG_BM * k + (author >> 5), bit);
          const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
          for (uint32_t c = 0; c < cn; c++)
            if (sup != DG_NO_SLOT && st.cand_slot[DG_CAND * k + c] == sup)
              atomicOr(st.vote + DG_BM * (DG_CAND * k + c) + (author >> 5), bit);
        }
      }
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_dg_cert(DagStore d, uint64_t nb, DecideIn in, DecideState st, uint64_t nvote,
                                                uint64_t ndec, const uint64_t* __restrict__ stakes, uint32_t n_auth,
                                                uint64_t quorum_thr, u64* __restrict__ ctl) {
  __shared__ uint32_t bms[WG / 64][DG_CAND][DG_BM];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t(*bm)[DG_BM] = bms[threadIdx.x / 64];
  uint64_t di, j, rec, k;
  bool bad = false;
  if (wave_task(d, nb, in, st.dlist, ndec, 2, &di, &j, &rec, &k, &bad)) {
    const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
    const uint32_t author = d.auth[rec];
    const uint64_t base = d.ibase[rec], vround = d.round[rec] - 1;
    const uint32_t kc = d.kc[rec];
    bad = base > d.cap_i || kc > d.cap_i - base;
    if (!bad && cn && author < n_auth && author < DG_MAX_AUTH) {
      for (uint32_t i = lane; i < DG_CAND * DG_BM; i += 64) (&bm[0][0])[i] = 0;
      wave_sync();
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {
        const uint32_t q = q0 + lane;
        if (q >= kc) continue;
        const u64 s = d.inc[base + q];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        const uint32_t v = d.map[s];  // an include without a record (seeded, pruned) votes for nothing
        if (v == DG_NONE) continue;
        if (v >= nb) {
          bad = true;
          continue;
        }
        const uint32_t va = d.auth[v], vp = st.vpos[v];
        if (d.round[v] != vround || va >= n_auth || va >= DG_MAX_AUTH || vp >= nvote) continue;
        const u64 sup = st.sup[(uint64_t)vp * in.gmax + j];  // (k_dg_vote's, an earlier launch)
        if (sup == DG_NO_SLOT) continue;
        for (uint32_t c = 0; c < cn; c++)
          if (st.cand_slot[DG_CAND * k + c] == sup) atomicOr(&bm[c][va >> 5], 1u << (va & 31));
      }
      wave_sync();
      uint32_t certifies = 0;
      for (uint32_t c = 0; c < cn; c++) {
        const uint64_t stake = bitmap_stake(bm[c], stakes, n_auth);
        if (stake > quorum_thr) certifies |= 1u << c;
        if (lane == 0 && stake > quorum_thr)
          atomicOr(st.cert + DG_BM * (DG_CAND * k + c) + (author >> 5), 1u << (author & 31));
      }
      if (st.cmask && lane == 0) st.cmask[di * in.gmax + j] = (uint8_t)certifies;  // (this wave's own byte; a commit call reads it)
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_dg_decide(const u64* __restrict__ slots, uint64_t n_slots, DecideIn in, DecideState st,
                                                  const uint64_t* __restrict__ stakes, uint32_t n_auth, uint64_t quorum_thr,
                                                  uint64_t* __restrict__ out, uint64_t* __restrict__ stakes_out,
                                                  u64* __restrict__ ctl) {
  const uint64_t k = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  const uint32_t lane = threadIdx.x & 63;
  if (k >= in.n) return;
  const uint64_t a = in.l_auth[k], r = in.l_round[k], row = in.l_row[k];
  if (row >= in.n) return;
  uint64_t w[8] = {a, r, 0, 0, 0, 0, MV_LEADER_UNDECIDED, 0}, sk[3] = {0, 0, 0};
  bool bad = false;
  if (a < n_auth) {
    const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
    const uint64_t blame = bitmap_stake(st.blame + DG_BM * k, stakes, n_auth);
    uint64_t best_v = 0, best_c = 0, com_v = 0, com_c = 0;
    u64 com_slot = DG_NO_SLOT;
    uint32_t enough = 0;
    for (uint32_t c = 0; c < cn; c++) {
      const uint64_t v = bitmap_stake(st.vote + DG_BM * (DG_CAND * k + c), stakes, n_auth);
      const uint64_t ce = bitmap_stake(st.cert + DG_BM * (DG_CAND * k + c), stakes, n_auth);
      if (v > best_v || (v == best_v && ce > best_c)) best_v = v, best_c = ce;
      if (ce > quorum_thr) enough++, com_v = v, com_c = ce, com_slot = st.cand_slot[DG_CAND * k + c];
    }
    const u64 nlo = ctl[mvk::IX_CTL_DG_NLO];  // max of ~round over the records, 0 without any
    uint64_t status = MV_LEADER_UNDECIDED;
    if (nlo == 0 || r < ~nlo) status = MV_LEADER_UNDECIDED;  // below the lowest retained round
    else if (blame > quorum_thr) status = MV_LEADER_SKIP;
    else if (found > DG_CAND) status = MV_LEADER_OVERFLOW;
    else if (enough == 1) status = MV_LEADER_COMMIT;
    else if (enough > 1) status = MV_LEADER_CONFLICT;
    if (status == MV_LEADER_COMMIT) {
      bad = com_slot >= n_slots;
      if (bad) status = MV_LEADER_UNDECIDED;
      else
        for (int i = 0; i < 6; i++) w[i] = slots[SLOT_WORDS * com_slot + 2 + i];
    }
    w[6] = status, w[7] = found;
    sk[0] = blame;
    if (found <= DG_CAND) sk[1] = enough == 1 ? com_v : best_v, sk[2] = enough == 1 ? com_c : best_c;
  }
  if (lane == 0) {
    for (int i = 0; i < 8; i++) out[8 * row + i] = w[i];
    if (stakes_out)
      for (int i = 0; i < 3; i++) stakes_out[3 * row + i] = sk[i];
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && lane == 0);
}

// ---------------------------------------------------------------- the indirect rule and the committed sequence
// mv_commit_leaders: BaseCommitter::try_indirect_decide (base_committer.rs:294-318) with
// decide_leader_from_anchor (:184-224) over BlockStore::linked_to_round (block_store.rs:306-327),
// and the prefix of UniversalCommitter::try_commit (universal_committer.rs:75-90), on top of the
// direct stages above, whose k_dg_cert also leaves the candidates every decision record certifies
// (DecideState::cmask). The rows stand in non-decreasing round order. The memory model is the
// file's: lanes of one launch talk only through agent-scope atomic read-modify-writes on single
// words (a job claimed by CAS, min / max on a job's words, OR into a mark bitmap, which is also
// read by an atomic OR of 0 where the same launch writes other bits of the word), nobody waits, and
// what a kernel reads as plain data an earlier launch wrote: the chain step reads fin[] and the out
// rows and writes act[]; only the resolve step, a later launch, writes fin[] and the out rows.
//   k_cm_init     a lane per row: rows the direct rule decided are final; the slot of a COMMIT row's block
//   k_cm_chain    a lane per row that is not final: the first row at least three rounds up that is
//                 not SKIP -- not final yet: wait for a later pass; COMMIT: the anchor, whose walk job
//                 is claimed once and takes the lowest target round; anything else: blocked
//   k_cm_seed     a lane per job: the anchor's record into the job's marks
//   k_cm_span_*   once per call: the records of the rounds a level can read, count / scan / list
//   k_cm_reach    one launch per level q some job passes, a wave per record of the span, at work when
//                 its round is q + 1: for every job whose walk passes the level and that marks
//                 it, the includes of key round q in batches of 64 -- with a record: marked; without: the
//                 job is incomplete from q up
//   k_cm_resolve  a wave per row the chain step moved: the marked decision records of round r + 2,
//                 their certificate masks, the incomplete tests, the verdict
//   k_cm_prefix   one wave: the sequence's length
using mvk::CommitState;

__device__ inline bool marked(const uint32_t* marks, uint64_t words, uint64_t id, uint64_t rec) {
  return (marks[id * words + (rec >> 5)] >> (rec & 31)) & 1u;
}

__global__ void __launch_bounds__(WG) k_cm_init(const u64* __restrict__ slots, uint64_t n_slots, DecideIn in, DecideState st,
                                                CommitState cs, const uint64_t* __restrict__ out,
                                                uint64_t* __restrict__ info, u64* __restrict__ ctl) {
  const uint64_t k = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (k < in.n) {
    const uint64_t status = out[8 * k + 6];
    u64 at = DG_NO_SLOT;
    if (status == MV_LEADER_COMMIT) {
      const uint32_t found = st.cand_n[k], cn = found < DG_CAND ? found : DG_CAND;
      for (uint32_t c = 0; c < cn; c++) {
        const u64 s = st.cand_slot[DG_CAND * k + c];
        if (s >= n_slots) continue;
        bool eq = true;
        for (int w = 0; w < 6; w++) eq &= slots[SLOT_WORDS * s + 2 + w] == out[8 * k + w];
        if (eq) at = s;
      }
      bad = at == DG_NO_SLOT;
    }
    const bool fin = status != MV_LEADER_UNDECIDED;
    cs.fin[k] = fin;
    cs.act[k] = mvk::CM_ACT_NONE;
    cs.anchor[k] = DG_NONE;
    cs.cslot[k] = at;
    info[4 * k] = fin ? 1 : 0, info[4 * k + 1] = ~0ull, info[4 * k + 2] = 0, info[4 * k + 3] = 0;
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_cm_chain(DecideIn in, CommitState cs, const uint64_t* __restrict__ out,
                                                 u64* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint32_t act = mvk::CM_ACT_NONE;
  if (i < in.n && !cs.fin[i]) {
    const uint64_t r = in.l_round[i];
    act = mvk::CM_ACT_UNDECIDED;
    if (r <= ~0ull - 3) {
      uint64_t lo = i + 1, hi = in.n;  // the first row of round >= r + 3
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (in.l_round[mid] < r + 3) lo = mid + 1;
        else hi = mid;
      }
      for (uint64_t j = lo; j < in.n; j++) {  // bounded by the rows
        if (!cs.fin[j]) {
          act = mvk::CM_ACT_NONE;  // decided by a later pass
          break;
        }
        const uint64_t status = out[8 * j + 6];
        if (status == MV_LEADER_SKIP) continue;
        if (status != MV_LEADER_COMMIT) {
          act = mvk::CM_ACT_BLOCKED;
          break;
        }
        act = mvk::CM_ACT_WALK;
        cs.anchor[i] = (uint32_t)j;
        if (atomicCAS(cs.job_id + j, DG_NONE, mvk::CM_CLAIMED) == DG_NONE) {
          const u64 id = atomicAdd(ctl + mvk::IX_CTL_CM_NJOBS, 1ull);
          if (id < in.n) {
            cs.jobs[id] = (uint32_t)j;
            atomicExch(cs.job_id + j, (uint32_t)id);
          }
        }
        atomicMin((u64*)cs.job_low + j, (u64)(r + 2));
        atomicMax(ctl + mvk::IX_CTL_CM_QHI, (u64)in.l_round[j]);
        atomicMax(ctl + mvk::IX_CTL_CM_NQLO, (u64)~(r + 2));
        break;
      }
    }
  }
  if (i < in.n) cs.act[i] = act;
  wave_count_to(ctl + mvk::IX_CTL_CM_MOVED, act != mvk::CM_ACT_NONE);
}

__global__ void __launch_bounds__(WG) k_cm_seed(DagStore d, uint64_t nb, uint64_t n, CommitState cs, uint64_t njobs,
                                                u64* __restrict__ ctl) {
  const uint64_t id = (uint64_t)blockIdx.x * WG + threadIdx.x;
  bool bad = false;
  if (id < njobs) {
    const uint64_t j = cs.jobs[id];
    const u64 s = j < n ? cs.cslot[j] : DG_NO_SLOT;
    const uint32_t rec = s < d.n_slots ? d.map[s] : DG_NONE;
    bad = rec >= nb || (rec >> 5) >= cs.mark_words;
    if (!bad) atomicOr(cs.marks + id * cs.mark_words + (rec >> 5), 1u << (rec & 31));
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

// the records of rounds lo..hi, the only ones a level of the call can read: count / scan / list
__device__ inline bool in_span(const DagStore& d, uint64_t nb, uint64_t rec, uint64_t lo, uint64_t hi) {
  return rec < nb && d.round[rec] >= lo && d.round[rec] <= hi;
}
__global__ void __launch_bounds__(WG) k_cm_span_count(DagStore d, uint64_t nb, uint64_t lo, uint64_t hi,
                                                      uint64_t* __restrict__ wgcount) {
  const uint64_t rec = (uint64_t)blockIdx.x * WG + threadIdx.x;
  uint64_t tot;
  (void)wg_excl(in_span(d, nb, rec, lo, hi), &tot);
  if (threadIdx.x == 0) wgcount[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(WG) k_cm_span_list(DagStore d, uint64_t nb, uint64_t lo, uint64_t hi,
                                                     const uint64_t* __restrict__ wgbase, uint32_t* __restrict__ span) {
  const uint64_t rec = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const bool in = in_span(d, nb, rec, lo, hi);
  uint64_t tot;
  const uint64_t at = wgbase[blockIdx.x] + wg_excl(in, &tot);
  if (in && at < nb) span[at] = (uint32_t)rec;
}

__global__ void __launch_bounds__(WG) k_cm_reach(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                 CommitState cs, uint64_t njobs, uint64_t nspan, uint64_t q,
                                                 u64* __restrict__ ctl) {
  const uint64_t w = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per record of the span
  const uint32_t lane = threadIdx.x & 63;
  if (w >= nspan) return;
  const uint64_t rec = cs.span[w];
  if (rec >= nb) {
    wave_count_to(ctl + mvk::IX_CTL_ERR, lane == 0);
    return;
  }
  if (d.round[rec] != q + 1 || (rec >> 5) >= cs.mark_words) return;
  const uint64_t base = d.ibase[rec];
  const uint32_t kc = d.kc[rec];
  bool bad = base > d.cap_i || kc > d.cap_i - base;
  if (!bad) {
    for (uint64_t id = 0; id < njobs; id++) {  // bounded by the jobs the host read back
      const uint64_t j = cs.jobs[id];
      if (j >= in.n) {
        bad = true;
        continue;
      }
      if (in.l_round[j] < q + 1 || cs.job_low[j] > q) continue;  // the job's walk does not pass this level
      // (this launch sets bits of round-q records in the same words: read through an atomic)
      uint32_t word = 0;
      if (lane == 0) word = atomicOr(cs.marks + id * cs.mark_words + (rec >> 5), 0u);
      word = (uint32_t)__shfl((int)word, 0);
      if (!((word >> (rec & 31)) & 1u)) continue;
      bool miss = false;
      for (uint32_t q0 = 0; q0 < kc; q0 += 64) {  // bounded by the include count; the wave stays together
        const uint32_t x = q0 + lane;
        if (x >= kc) continue;
        const u64 s = d.inc[base + x];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        if (slots[SLOT_WORDS * s + 3] != q) continue;  // a weak link leads nowhere (block_store.rs:312-321)
        const uint32_t v = d.map[s];
        if (v == DG_NONE) miss = true;
        else if (v >= nb || (v >> 5) >= cs.mark_words) bad = true;
        else atomicOr(cs.marks + id * cs.mark_words + (v >> 5), 1u << (v & 31));
      }
      if (__ballot(miss) != 0 && lane == 0) atomicMax((u64*)cs.job_miss + j, (u64)(q + 1));
    }
  }
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad);
}

__global__ void __launch_bounds__(WG) k_cm_resolve(const u64* __restrict__ slots, DagStore d, uint64_t nb, DecideIn in,
                                                   DecideState st, CommitState cs, uint64_t nvote, uint64_t ndec,
                                                   uint64_t njobs, uint64_t* __restrict__ out, uint64_t* __restrict__ info,
                                                   u64* __restrict__ ctl) {
  const uint64_t i = ((uint64_t)blockIdx.x * WG + threadIdx.x) / 64;  // a wave per row
  const uint32_t lane = threadIdx.x & 63;
  if (i >= in.n) return;
  const uint32_t act = cs.act[i];
  if (act == mvk::CM_ACT_NONE) return;
  if (act != mvk::CM_ACT_WALK) {
    if (lane == 0) {
      cs.fin[i] = 1;
      info[4 * i + 2] = act == mvk::CM_ACT_BLOCKED ? 2 : 0;
    }
    return;
  }
  const uint64_t r = in.l_round[i], j = cs.anchor[i];
  const uint64_t id = j < in.n ? cs.job_id[j] : DG_NONE;
  uint64_t g = 0;
  bool bad = id >= njobs || !leader_group(in, r, &g) || i < in.g_start[g] || i - in.g_start[g] >= in.gmax;
  uint32_t mask = 0;
  uint64_t count = 0;
  bool incomplete = false;
  if (!bad) {
    const uint64_t jrow = i - in.g_start[g];
    for (uint64_t di = lane; di < ndec; di += 64) {  // bounded by the decision records the host read back
      const uint32_t rec = st.dlist[di];
      if (rec >= nb || (rec >> 5) >= cs.mark_words) {
        bad = true;
        continue;
      }
      if (d.round[rec] != r + 2 || !marked(cs.marks, cs.mark_words, id, rec)) continue;
      count++;
      mask |= st.cmask[di * in.gmax + jrow];
      const uint64_t base = d.ibase[rec];
      const uint32_t kc = d.kc[rec];
      if (base > d.cap_i || kc > d.cap_i - base) {
        bad = true;
        continue;
      }
      for (uint32_t x = 0; x < kc; x++) {  // a voting block without a record, or one whose support has none
        const u64 s = d.inc[base + x];
        if (s >= d.n_slots) {
          bad = true;
          continue;
        }
        if (slots[SLOT_WORDS * s + 3] != r + 1) continue;
        const uint32_t v = d.map[s];
        if (v == DG_NONE) {
          incomplete = true;
          continue;
        }
        const uint32_t vp = v < nb ? st.vpos[v] : DG_NONE;
        if (vp >= nvote) continue;
        const u64 sup = st.sup[(uint64_t)vp * in.gmax + jrow];
        if (sup == DG_NO_SLOT) continue;
        if (sup >= d.n_slots) bad = true;
        else if (d.map[sup] == DG_NONE) incomplete = true;
      }
    }
  }
  for (int w = 32; w; w >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, w);
  count = wave_sum64(count);
  incomplete = __ballot(incomplete) != 0;
  bad = __ballot(bad) != 0;
  if (lane == 0 && !bad) {
    const u64 nlo = ctl[mvk::IX_CTL_DG_NLO];  // (written by a connect call or a prune, earlier launches)
    incomplete = incomplete || nlo == 0 || r < ~nlo || cs.job_miss[j] >= r + 3;
    const uint32_t found = st.cand_n[i], cn = found < DG_CAND ? found : DG_CAND;
    mask &= (1u << cn) - 1;
    const int ncert = __popc(mask);
    uint64_t status = MV_LEADER_UNDECIDED, kind = 2;
    u64 com = DG_NO_SLOT;
    if (found > DG_CAND) status = MV_LEADER_OVERFLOW;  // (defensive: the direct rule already ended such a row)
    else if (ncert == 1) status = MV_LEADER_COMMIT, com = st.cand_slot[DG_CAND * i + (__ffs((int)mask) - 1)];
    else if (ncert > 1) status = MV_LEADER_CONFLICT;
    else if (incomplete) kind = 0;
    else status = MV_LEADER_SKIP;
    if (status == MV_LEADER_COMMIT) {
      if (com >= d.n_slots) bad = true;
      else
        for (int w = 0; w < 6; w++) out[8 * i + w] = slots[SLOT_WORDS * com + 2 + w];
    }
    if (!bad) {
      out[8 * i + 6] = status;
      cs.cslot[i] = com;
      info[4 * i] = kind, info[4 * i + 1] = j, info[4 * i + 2] = incomplete ? 1 : 0, info[4 * i + 3] = count;
    }
  }
  if (lane == 0) cs.fin[i] = 1;
  wave_count_to(ctl + mvk::IX_CTL_ERR, bad && lane == 0);
}

__global__ void __launch_bounds__(64) k_cm_prefix(DecideIn in, const uint64_t* __restrict__ out, u64* __restrict__ ctl) {
  const uint32_t lane = threadIdx.x;
  uint64_t first = in.n, zero = 0;
  for (uint64_t i = lane; i < in.n; i += 64) {  // bounded by the rows
    if (in.l_round[i] == 0) {
      zero++;
      continue;
    }
    const uint64_t status = out[8 * i + 6];
    if (status != MV_LEADER_COMMIT && status != MV_LEADER_SKIP && i < first) first = i;
  }
  for (int w = 32; w; w >>= 1) {
    const uint64_t o = shfl64(first, lane ^ w);
    first = o < first ? o : first;
  }
  zero = wave_sum64(zero);
  if (lane == 0) atomicExch(ctl + mvk::IX_CTL_CM_NSEQ, (u64)(first >= zero ? first - zero : 0));
}

static inline uint32_t grid_of(uint64_t items) { return (uint32_t)((items + WG - 1) / WG); }

}  // namespace ix
}  // namespace mv

namespace mvk {

using namespace mv::ix;

uint64_t index_groups(uint64_t n) { return (n + WG - 1) / WG; }

hipError_t launch_index_scan(const uint64_t* wgcount, uint64_t nwg, uint64_t* wgbase, uint64_t* total, hipStream_t s) {
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wgcount, nwg, wgbase, total);
  return hipGetLastError();
}

hipError_t launch_index_round(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint64_t* item, uint32_t state,
                              int round, uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  u64* c = (u64*)ctl;
  const dim3 g(grid_of(n)), b(WG);
  hipLaunchKernelGGL(k_ix_claim, g, b, 0, s, t, ks, n, (u64*)item, state, round, c);
  hipLaunchKernelGGL(k_ix_fill, g, b, 0, s, t, ks, n, (u64*)item, state, c);
  hipLaunchKernelGGL(k_ix_settle, g, b, 0, s, t, ks, n, (u64*)item, c);
  return hipGetLastError();
}

hipError_t launch_index_giveup(uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_ix_giveup, dim3(1), dim3(64), 0, s, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_prior(const uint64_t* item, uint64_t n, uint8_t* prior, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_prior, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)item, n, prior);
  return hipGetLastError();
}

hipError_t launch_index_lookup(const IndexTable& t, const IndexKeys& ks, uint64_t n, uint8_t* out, uint64_t* ctl,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_lookup, dim3(grid_of(n)), dim3(WG), 0, s, t, ks, n, out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_rebuild(const uint64_t* old_slots, uint64_t n_old, const IndexTable& t, uint64_t* ctl,
                                hipStream_t s) {
  if (n_old == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ix_rebuild, dim3(grid_of(n_old)), dim3(WG), 0, s, (const u64*)old_slots, n_old, t, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_index_wanted(const IndexTable& t, uint64_t* wgcount, uint64_t* wgbase, uint64_t* total, uint64_t* out,
                               uint64_t cap, hipStream_t s) {
  const uint64_t n = t.mask + 1;
  const dim3 g(grid_of(n)), b(WG);
  hipLaunchKernelGGL(k_ix_wanted_count, g, b, 0, s, (const u64*)t.slots, n, wgcount);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wgcount, index_groups(n), wgbase, total);
  if (cap) hipLaunchKernelGGL(k_ix_wanted_list, g, b, 0, s, (const u64*)t.slots, n, wgbase, out, cap);
  return hipGetLastError();
}

hipError_t launch_accept_probe(const IndexTable& t, const AcceptArrays& a, uint64_t* ctl, hipStream_t s) {
  const dim3 g(grid_of(a.n)), b(WG);
  hipLaunchKernelGGL(k_acc_probe, g, b, 0, s, t, a, (u64*)ctl);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, a.wg_a, index_groups(a.n), a.base_a, ctl + IX_CTL_NVER);
  hipLaunchKernelGGL(k_acc_vlist, g, b, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_accept_groups(const AcceptArrays& a, uint64_t* ctl, hipStream_t s) {
  const dim3 g(grid_of(a.n)), b(WG);
  const uint64_t nwg = index_groups(a.n);
  if (a.grp) {
    hipLaunchKernelGGL(k_acc_heads, g, b, 0, s, a);
    hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, a.wg_a, nwg, a.base_a, ctl + IX_CTL_NHEADS);
  }
  hipLaunchKernelGGL(k_acc_groups, g, b, 0, s, a);
  hipLaunchKernelGGL(k_acc_states, g, b, 0, s, a);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, a.wg_a, nwg, a.base_a, ctl + IX_CTL_NCAND);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, a.wg_b, nwg, a.base_b, ctl + IX_CTL_NINC);
  hipLaunchKernelGGL(k_acc_cand_list, g, b, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_accept_own_states(const AcceptArrays& a, const uint64_t* item, uint64_t ncand, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_acc_own_states, dim3(grid_of(ncand)), dim3(WG), 0, s, a, (const u64*)item, ncand);
  return hipGetLastError();
}

hipError_t launch_accept_inc_src(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, uint64_t* inc_src, hipStream_t s) {
  if (ninc == 0 || ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_acc_inc_src, dim3(grid_of(ninc)), dim3(WG), 0, s, a, ncand, ninc, inc_src);
  return hipGetLastError();
}

hipError_t launch_accept_missing(const IndexTable& t, const uint64_t* item, uint64_t ninc, uint64_t* wgcount,
                                 uint64_t* wgbase, uint64_t* ctl, uint64_t* out, uint64_t cap, hipStream_t s) {
  if (ninc == 0) return hipSuccess;
  const dim3 g(grid_of(ninc)), b(WG);
  hipLaunchKernelGGL(k_acc_miss_count, g, b, 0, s, (const u64*)item, ninc, wgcount);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wgcount, index_groups(ninc), wgbase, ctl + IX_CTL_NMISS);
  if (cap) hipLaunchKernelGGL(k_acc_miss_list, g, b, 0, s, t, (const u64*)item, ninc, wgbase, out, cap);
  return hipGetLastError();
}

hipError_t launch_pend_own_slots(const uint64_t* item, uint64_t ncand, uint64_t* cand_slot, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_own_slots, dim3(grid_of(ncand)), dim3(WG), 0, s, (const u64*)item, ncand, cand_slot);
  return hipGetLastError();
}

hipError_t launch_pend_append(const AcceptArrays& a, uint64_t ncand, uint64_t ninc, const uint64_t* item,
                              const uint64_t* cand_slot, uint64_t* cand_dst, const PendStore& p, uint64_t nb0, uint64_t ni0,
                              uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (ncand == 0) return hipSuccess;
  const uint64_t nwg = index_groups(ncand);
  uint64_t *wg_a = wg, *wg_b = wg + nwg, *base_a = wg + 2 * nwg, *base_b = wg + 3 * nwg;
  const dim3 g(grid_of(ncand)), b(WG);
  hipLaunchKernelGGL(k_pb_app_count, g, b, 0, s, a, ncand, wg_a, wg_b);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_a, nwg, base_a, ctl + IX_CTL_PB_NB);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_b, nwg, base_b, ctl + IX_CTL_PB_NI);
  hipLaunchKernelGGL(k_pb_app_list, g, b, 0, s, a, ncand, cand_slot, base_a, base_b, p, nb0, ni0, cand_dst);
  if (ninc) hipLaunchKernelGGL(k_pb_app_inc, dim3(grid_of(ninc)), b, 0, s, a, ncand, ninc, (const u64*)item, cand_dst, p);
  return hipGetLastError();
}

hipError_t launch_pend_level(const IndexTable& t, const PendStore& p, uint64_t nb, uint32_t* lvl, uint8_t* hit,
                             uint64_t level, uint64_t* wg, uint64_t* out, uint64_t cap, uint64_t* ctl, int lv_word,
                             uint32_t* row_of, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_pb_check, dim3(grid_of(64 * nb)), b, 0, s, (const u64*)t.slots, p, nb, lvl, hit);
  hipLaunchKernelGGL(k_pb_count, g, b, 0, s, hit, nb, wg);
  hipLaunchKernelGGL(k_pb_scan, dim3(1), dim3(1024), 0, s, wg, nwg, wg + nwg, ctl + IX_CTL_PB_ROWS, ctl + lv_word);
  hipLaunchKernelGGL(k_pb_list, g, b, 0, s, (u64*)t.slots, p, nb, hit, wg + nwg, lvl, level, out, cap, (u64*)ctl, row_of);
  return hipGetLastError();
}

hipError_t launch_pend_compact(const IndexTable& t, const PendStore& p, const PendStore& q, uint64_t nb, uint64_t* newbase,
                               uint8_t* state, uint64_t n_state, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  uint64_t *wg_a = wg, *wg_b = wg + nwg, *base_a = wg + 2 * nwg, *base_b = wg + 3 * nwg;
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_pb_keep_count, g, b, 0, s, (const u64*)t.slots, p, nb, wg_a, wg_b);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_a, nwg, base_a, ctl + IX_CTL_PB_NB);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_b, nwg, base_b, ctl + IX_CTL_PB_NI);
  hipLaunchKernelGGL(k_pb_keep_list, g, b, 0, s, (const u64*)t.slots, p, q, nb, base_a, base_b, newbase, state, state ? n_state : 0);
  hipLaunchKernelGGL(k_pb_keep_inc, dim3(grid_of(64 * nb)), b, 0, s, p, q, nb, newbase);
  return hipGetLastError();
}

hipError_t launch_pend_reresolve(const uint64_t* old_slots, const IndexTable& t, uint64_t* slotidx, uint64_t n,
                                 uint64_t* ctl, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_reresolve, dim3(grid_of(n)), dim3(WG), 0, s, (const u64*)old_slots, t, slotidx, n, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_dag_append(const IndexTable& t, const PendStore& p, uint64_t nb, const uint32_t* lvl,
                             const uint32_t* row_of, uint64_t rows, const DagStore& d, uint64_t nb0, uint64_t ni0,
                             uint64_t* src, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (rows == 0 || nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(rows);
  const dim3 gr(grid_of(rows)), b(WG);
  hipError_t e = hipMemsetAsync(src, 0xff, 8 * rows, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_dg_app_rows, dim3(grid_of(nb)), b, 0, s, (const u64*)t.slots, p, nb, lvl, row_of, rows, d, nb0, src,
                     (u64*)ctl);
  hipLaunchKernelGGL(k_dg_app_count, gr, b, 0, s, d, nb0, rows, src, wg);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg, nwg, wg + nwg, ctl + IX_CTL_DG_NI);
  hipLaunchKernelGGL(k_dg_app_list, gr, b, 0, s, d, nb0, ni0, rows, src, wg + nwg);
  hipLaunchKernelGGL(k_dg_app_inc, dim3(grid_of(64 * rows)), b, 0, s, p, nb, d, nb0, rows, src, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_dag_map(const DagStore& d, uint64_t nb, uint64_t* ctl, hipStream_t s) {
  if (d.n_slots == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(d.map, 0xff, 4 * d.n_slots, s);
  if (e != hipSuccess || nb == 0) return e;
  hipLaunchKernelGGL(k_dg_map, dim3(grid_of(nb)), dim3(WG), 0, s, d, nb, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_dag_prune(const DagStore& d, const DagStore& q, uint64_t nb, uint64_t floor, uint64_t* newbase,
                            uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  uint64_t *wg_a = wg, *wg_b = wg + nwg, *base_a = wg + 2 * nwg, *base_b = wg + 3 * nwg;
  const dim3 g(grid_of(nb)), b(WG);
  hipError_t e = hipMemsetAsync(q.map, 0xff, 4 * q.n_slots, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_dg_keep_count, g, b, 0, s, d, nb, floor, wg_a, wg_b);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_a, nwg, base_a, ctl + IX_CTL_DG_NB);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_b, nwg, base_b, ctl + IX_CTL_DG_NI);
  hipLaunchKernelGGL(k_dg_keep_list, g, b, 0, s, d, q, nb, floor, base_a, base_b, newbase, (u64*)ctl);
  hipLaunchKernelGGL(k_dg_keep_inc, dim3(grid_of(64 * nb)), b, 0, s, d, q, nb, newbase);
  return hipGetLastError();
}

hipError_t launch_seed_eligible(const SeedRows& r, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (r.n == 0) return hipSuccess;
  const uint64_t nwg = index_groups(r.n);
  hipLaunchKernelGGL(k_sd_elig, dim3(grid_of(r.n)), dim3(WG), 0, s, r, wg, wg + nwg, (u64*)ctl);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg, nwg, wg + 2 * nwg, ctl + IX_CTL_SD_ELIG);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg + nwg, nwg, wg + 3 * nwg, ctl + IX_CTL_SD_EINC);
  return hipGetLastError();
}

hipError_t launch_seed_records(const IndexTable& t, const uint64_t* item, const SeedRows& r, const DagStore& d, uint64_t nb0,
                               uint64_t ni0, uint64_t* wg, uint64_t* ctl, hipStream_t s) {
  if (r.n == 0) return hipSuccess;
  const uint64_t nwg = index_groups(r.n);
  uint64_t *wg_a = wg, *wg_b = wg + nwg, *base_a = wg + 2 * nwg, *base_b = wg + 3 * nwg;
  const dim3 g(grid_of(r.n)), b(WG);
  hipLaunchKernelGGL(k_sd_claim, g, b, 0, s, (const u64*)item, r, d, nb0, (u64*)ctl);
  hipLaunchKernelGGL(k_sd_count, g, b, 0, s, r, d, nb0, wg_a, wg_b);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_a, nwg, base_a, ctl + IX_CTL_SD_NREC);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_b, nwg, base_b, ctl + IX_CTL_SD_NINC);
  hipLaunchKernelGGL(k_sd_list, g, b, 0, s, (const u64*)t.slots, r, d, nb0, ni0, base_a, base_b, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_seed_inc_src(const SeedRows& r, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                               uint64_t* inc_src, uint64_t* ctl, hipStream_t s) {
  if (nrec == 0 || ninc == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(inc_src, 0xff, 8 * ninc, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sd_inc_src, dim3(grid_of(64 * nrec)), dim3(WG), 0, s, r, d, nb0, ni0, nrec, ninc, inc_src, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_seed_inc(const uint64_t* item, const DagStore& d, uint64_t nb0, uint64_t ni0, uint64_t nrec, uint64_t ninc,
                           uint64_t* ctl, hipStream_t s) {
  if (nrec == 0 || ninc == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sd_inc, dim3(grid_of(64 * nrec)), dim3(WG), 0, s, (const u64*)item, d, nb0, ni0, nrec, ninc, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_decide_pick(const DagStore& d, uint64_t nb, const DecideIn& in, const DecideState& st, uint64_t* wg,
                              uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  uint64_t *wg_a = wg, *wg_b = wg + nwg, *base_a = wg + 2 * nwg, *base_b = wg + 3 * nwg;
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_dg_pick_count, g, b, 0, s, d, nb, in, wg_a, wg_b);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_a, nwg, base_a, ctl + IX_CTL_DG_NVOTE);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg_b, nwg, base_b, ctl + IX_CTL_DG_NDEC);
  hipLaunchKernelGGL(k_dg_pick_list, g, b, 0, s, d, nb, in, st, base_a, base_b);
  return hipGetLastError();
}

hipError_t launch_decide_rule(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                              const DecideState& st, uint64_t nvote, uint64_t ndec, const uint64_t* stakes,
                              uint32_t n_auth, uint64_t quorum_thr, uint64_t* out, uint64_t* stakes_out, uint64_t* ctl,
                              hipStream_t s) {
  if (n_auth > DG_MAX_AUTH) return hipErrorInvalidValue;
  const dim3 b(WG);
  if (nvote) {
    hipError_t e = hipMemsetAsync(st.sup, 0xff, 8 * nvote * in.gmax, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dg_vote, dim3(grid_of(64 * nvote * in.gmax)), b, 0, s, (const u64*)t.slots, d, nb, in, st, nvote,
                       (u64*)ctl);
  }
  if (ndec && nvote)
    hipLaunchKernelGGL(k_dg_cert, dim3(grid_of(64 * ndec * in.gmax)), b, 0, s, d, nb, in, st, nvote, ndec, stakes, n_auth,
                       quorum_thr, (u64*)ctl);
  hipLaunchKernelGGL(k_dg_decide, dim3(grid_of(64 * in.n)), b, 0, s, (const u64*)t.slots, d.n_slots, in, st, stakes, n_auth,
                     quorum_thr, out, stakes_out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_init(const IndexTable& t, const DecideIn& in, const DecideState& st, const CommitState& cs,
                              const uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_init, dim3(grid_of(in.n)), dim3(WG), 0, s, (const u64*)t.slots, t.mask + 1, in, st, cs, out, info,
                     (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_chain(const DecideIn& in, const CommitState& cs, const uint64_t* out, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_chain, dim3(grid_of(in.n)), dim3(WG), 0, s, in, cs, out, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_span(const DagStore& d, uint64_t nb, uint64_t lo, uint64_t hi, uint32_t* span, uint64_t* wg,
                              uint64_t* ctl, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  const uint64_t nwg = index_groups(nb);
  const dim3 g(grid_of(nb)), b(WG);
  hipLaunchKernelGGL(k_cm_span_count, g, b, 0, s, d, nb, lo, hi, wg);
  hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(1024), 0, s, wg, nwg, wg + nwg, ctl + IX_CTL_CM_NSPAN);
  hipLaunchKernelGGL(k_cm_span_list, g, b, 0, s, d, nb, lo, hi, wg + nwg, span);
  return hipGetLastError();
}

hipError_t launch_commit_reach(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                               const CommitState& cs, uint64_t njobs, uint64_t nspan, const uint64_t* levels,
                               uint64_t n_levels, uint64_t* ctl, hipStream_t s) {
  if (njobs == 0 || nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cm_seed, dim3(grid_of(njobs)), dim3(WG), 0, s, d, nb, in.n, cs, njobs, (u64*)ctl);
  if (nspan == 0) return hipGetLastError();
  for (uint64_t k = 0; k < n_levels; k++)  // downwards
    hipLaunchKernelGGL(k_cm_reach, dim3(grid_of(64 * nspan)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, in, cs, njobs, nspan,
                       levels[k], (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_resolve(const IndexTable& t, const DagStore& d, uint64_t nb, const DecideIn& in,
                                 const DecideState& st, const CommitState& cs, uint64_t nvote, uint64_t ndec, uint64_t njobs,
                                 uint64_t* out, uint64_t* info, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_resolve, dim3(grid_of(64 * in.n)), dim3(WG), 0, s, (const u64*)t.slots, d, nb, in, st, cs, nvote,
                     ndec, njobs, out, info, (u64*)ctl);
  return hipGetLastError();
}

hipError_t launch_commit_prefix(const DecideIn& in, const uint64_t* out, uint64_t* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_cm_prefix, dim3(1), dim3(64), 0, s, in, out, (u64*)ctl);
  return hipGetLastError();
}

}  // namespace mvk
