// The statement walk of the transaction votes (votes.hip: k_vt_scan, k_vt_emit): the include count
// that places a second reader at a parsed block's statements, a reference's index key, and the
// walk over the statements themselves. Every read goes through bincode_walk.h's BcReader. Plain
// C++ without device intrinsics: with MV_DEV and MV_VT_DEV defined as host function attributes it
// compiles for the host, where tools/walk_san.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#include "bincode_walk.h"

#ifndef MV_VT_DEV
#define MV_VT_DEV __device__ inline
#endif

namespace mv::ix {

// counts the includes; everything else of the walk is of no interest here
struct IncCount {
  uint64_t n_inc = 0;
  MV_DEV void own(uint64_t, uint64_t, const uint8_t*) {}
  MV_DEV void include(uint64_t, uint64_t, const uint8_t*) { n_inc++; }
  MV_DEV void vote_range(uint64_t, uint64_t) {}
  MV_DEV void meta(uint64_t, uint64_t) {}
};

MV_VT_DEV void ref_key(uint64_t a, uint64_t rd, const uint8_t* d, uint64_t k[6]) {
  k[0] = a, k[1] = rd;
#pragma unroll
  for (int w = 0; w < 4; w++) k[2 + w] = peek8(d + 8 * w);
}

// The statements of a block (types.rs:100-114), r standing at their count. f sees share(k),
// vote(k, key, offset) for an Accept, reject(k), range(k, key, start, end). Every read is checked by r.
template <class F>
MV_VT_DEV bool walk_statements(BcReader& r, F& f, uint64_t* count) {
  const uint64_t n_st = r.u64();
  if (r.ok && n_st > (r.len - r.pos) / 12) r.ok = false;
  *count = n_st;
  for (uint64_t k = 0; r.ok && k < n_st; k++) {
    const uint32_t tag = r.u32();
    if (!r.ok) break;
    uint64_t a, rd, key[6];
    const uint8_t* d;
    if (tag == 0) {
      const uint64_t l = r.u64();
      if (!r.take(l)) break;
      r.pos += l;
      f.share(k);
    } else if (tag == 1) {
      r.ref(a, rd, d);
      const uint64_t lo = r.u64();
      const uint32_t vote = r.u32();
      if (!r.ok) break;
      if (vote == 0) {
        ref_key(a, rd, d, key);
        f.vote(k, key, lo);
      } else if (vote == 1) {
        const uint32_t some = r.u8();
        if (!r.ok) break;
        if (some == 1) {
          r.ref(a, rd, d);
          (void)r.u64();
          if (!r.ok) break;
        } else if (some != 0) {
          r.ok = false;
          break;
        }
        f.reject(k);
      } else {
        r.ok = false;
      }
    } else if (tag == 2) {
      r.ref(a, rd, d);
      const uint64_t s0 = r.u64(), s1 = r.u64();
      if (!r.ok) break;
      ref_key(a, rd, d, key);
      f.range(k, key, s0, s1);
    } else {
      r.ok = false;
    }
  }
  return r.ok;
}

}  // namespace mv::ix
