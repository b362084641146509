// The rules of StatementBlock::verify that every ingest form applies, each stated once, and the
// per-block verdict (types.rs:315-376) from the ingest facts, the
// claimed and computed digests and the signature status: k_block_verdict (ingest.hip) and,
// fused into their last wave, the committee comb kernels of the online path (comb.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mysti_verify.h"

#ifndef MV_DEV
#define MV_DEV __device__ __forceinline__
#endif

namespace mv {

constexpr uint32_t BF_PARSED = 1u, BF_EPOCH_OK = 2u, BF_AUTHOR_OK = 4u, BF_GENESIS = 8u, BF_QUORUM = 32u;
constexpr int BF_INC_SHIFT = 8;  // first failing include: MV_BLOCK_INCLUDE_* or 0
constexpr int BF_VR_SHIFT = 16;  // first failing VoteRange: vr_code() or 0

struct CommitteeView {
  const uint64_t* stakes;
  uint32_t n_auth;
  uint64_t epoch, quorum_thr;
};

// The rules every ingest form applies while it reads a block (ingest_dev.h's one-lane walk and
// wave form, block_walk.hip), each stated once.
//
// An include's check (types.rs:349-362): the authority is known, the round is below the block's.
MV_DEV uint32_t include_code(uint64_t a, uint64_t r, uint64_t me_r, uint32_t n_auth) {
  return a >= n_auth ? (uint32_t)MV_BLOCK_INCLUDE_UNKNOWN_AUTHORITY : (r >= me_r ? (uint32_t)MV_BLOCK_INCLUDE_ROUND : 0u);
}
// The includes whose authorities' stake the threshold clock counts (threshold_clock.rs:12-35)
MV_DEV bool clock_include(uint64_t a, uint64_t r, uint64_t me_r, uint32_t n_auth) {
  return me_r > 0 && r == me_r - 1 && a < n_auth;
}
constexpr uint64_t VR_MAX_LEN = 1024 * 1024;  // VoteRange::verify MAX_LEN (types.rs:448)
// VoteRange::verify (types.rs:440-460), its checks in order: 1 = end < start, 2 = length
// >= MAX_LEN, 3 = end >= MAX_LEN, 0 = valid
MV_DEV uint32_t vr_code(uint64_t s0, uint64_t s1) {
  return s1 < s0 ? 1u : (s1 - s0 >= VR_MAX_LEN ? 2u : (s1 >= VR_MAX_LEN ? 3u : 0u));
}
// The facts word of a block that parsed (inc, vr: the first failing include's and VoteRange's code)
MV_DEV uint32_t block_facts(bool epoch_ok, bool author_ok, bool genesis, uint32_t vr, bool quorum, uint32_t inc) {
  return BF_PARSED | (epoch_ok ? BF_EPOCH_OK : 0u) | (author_ok ? BF_AUTHOR_OK : 0u) | (genesis ? BF_GENESIS : 0u) |
         (vr << BF_VR_SHIFT) | (quorum ? BF_QUORUM : 0u) | (inc << BF_INC_SHIFT);
}
// whether block_verdict() reaches the signature check
MV_DEV bool sig_decides(uint32_t f) {
  return (f & BF_PARSED) && (f & BF_EPOCH_OK) && (f & BF_AUTHOR_OK) && !(f & BF_GENESIS);
}
// The signature words (zero for a block that did not parse) to the verify stage. A block rejected
// ahead of the signature check gets s = 2^256 - 1 (>= l): its verdict does not depend on the
// signature, and s >= l keeps it out of the batch equation.
MV_DEV void store_sig(uint8_t* sig_out, uint32_t i, uint32_t (&sw)[16], uint32_t f) {
  if (!sig_decides(f)) {
#pragma unroll
    for (int q = 8; q < 16; q++) sw[q] = 0xffffffffu;
  }
  uint4* so4 = reinterpret_cast<uint4*>(sig_out + 64 * (size_t)i);
#pragma unroll
  for (int q = 0; q < 4; q++) so4[q] = make_uint4(sw[4 * q], sw[4 * q + 1], sw[4 * q + 2], sw[4 * q + 3]);
}
// the committee key a block's signature is checked against (0 where none is)
MV_DEV uint32_t block_key(uint32_t f, uint32_t author) {
  return (f & BF_PARSED) && (f & BF_AUTHOR_OK) ? author : 0u;
}
// What an ingest leaves per block for the hash, verify and verdict stages. claimed(q): 64-bit word
// q of the own reference's digest, called only for a block that parsed.
template <class ClaimedFn>
MV_DEV void store_block_outputs(uint32_t i, uint32_t f, uint32_t author, uint32_t (&sw)[16], ClaimedFn claimed,
                                uint8_t* sig_out, uint8_t* claimed_out, uint32_t* key_idx, uint32_t* facts) {
  store_sig(sig_out, i, sw, f);
  if (f & BF_PARSED) {
    uint4* cd = reinterpret_cast<uint4*>(claimed_out + 32 * (size_t)i);
    const uint64_t d0 = claimed(0), d1 = claimed(1), d2 = claimed(2), d3 = claimed(3);
    cd[0] = make_uint4((uint32_t)d0, (uint32_t)(d0 >> 32), (uint32_t)d1, (uint32_t)(d1 >> 32));
    cd[1] = make_uint4((uint32_t)d2, (uint32_t)(d2 >> 32), (uint32_t)d3, (uint32_t)(d3 >> 32));
  }
  key_idx[i] = block_key(f, author);
  facts[i] = f;
}

MV_DEV bool digest_same(const uint8_t* claimed, const uint8_t* digest, uint32_t i) {
  const uint4* a = reinterpret_cast<const uint4*>(claimed + 32 * (size_t)i);
  const uint4* b = reinterpret_cast<const uint4*>(digest + 32 * (size_t)i);
  const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) |
          (a1.z ^ b1.z) | (a1.w ^ b1.w)) == 0;
}

// status of block i in the order of StatementBlock::verify. A block that does not deserialize
// has no pre-image: its two digests are zeroed, so every output is deterministic.
MV_DEV uint8_t block_verdict(const uint32_t* facts, const uint8_t* claimed, uint8_t* msg_digest, uint8_t* digest,
                             uint8_t sig_status, uint32_t i) {
  const uint32_t f = facts[i];
  if (!(f & BF_PARSED)) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    uint4* m4 = reinterpret_cast<uint4*>(msg_digest + 32 * (size_t)i);
    uint4* d4 = reinterpret_cast<uint4*>(digest + 32 * (size_t)i);
    m4[0] = z;
    m4[1] = z;
    d4[0] = z;
    d4[1] = z;
    return MV_BLOCK_PARSE_ERROR;
  }
  const bool same = digest_same(claimed, digest, i);
  const uint32_t inc = (f >> BF_INC_SHIFT) & 0xffu;
  const uint32_t vr = (f >> BF_VR_SHIFT) & 3u;
  return !same                     ? MV_BLOCK_DIGEST_MISMATCH
         : !(f & BF_EPOCH_OK)      ? MV_BLOCK_EPOCH_MISMATCH
         : !(f & BF_AUTHOR_OK)     ? MV_BLOCK_UNKNOWN_AUTHOR
         : (f & BF_GENESIS)        ? MV_BLOCK_GENESIS
         : sig_status != MV_SIG_OK ? MV_BLOCK_SIG_INVALID
         : inc                     ? (uint8_t)inc
         : vr == 1                 ? MV_BLOCK_VOTE_RANGE
         : vr == 2                 ? MV_BLOCK_VOTE_RANGE_TOO_LONG
         : vr == 3                 ? MV_BLOCK_VOTE_RANGE_END_TOO_LARGE
         : !(f & BF_QUORUM)        ? MV_BLOCK_THRESHOLD_CLOCK
                                   : MV_BLOCK_OK;
}

}  // namespace mv
