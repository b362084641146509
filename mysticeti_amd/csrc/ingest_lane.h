// The one-lane verify ingest of a block: the shared walk (bincode_walk.h) under the verify checks
// (block_verdict.h), writing P || sig to the stage. Device code includes it through ingest_dev.h
// (ingest.hip's kernels and comb.hip's k_verify_comb16); like the walk it is plain C++ without device
// intrinsics, so with MV_DEV defined as a host function attribute it compiles for the host, where
// tools/walk_san.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#include "bincode_walk.h"
#include "block_verdict.h"

namespace mv {

// pre-image writer: the walk's bytes as aligned 64-bit stores to the stage
struct PreWriter : ByteGather<PreWriter> {
  uint64_t* out;
  MV_DEV explicit PreWriter(uint64_t* o) : out(o) {}
  MV_DEV void word(uint64_t w) { *out++ = w; }
  MV_DEV void flush() {
    if (nb) *out++ = acc;
    acc = 0;
    nb = 0;
  }
};

// Outputs of the ingest of one block (all indexed by block).
struct IngestOut {
  uint8_t* stage;
  uint64_t* pre_off;
  uint64_t* pre_len;
  uint8_t* sig_out;
  uint32_t* key_idx;
  uint32_t* facts;
  uint8_t* claimed;
};

// What the verify ingest gathers on the walk: the include checks (types.rs:349-362), the
// threshold clock's stake of the distinct round r-1 authorities (threshold_clock.rs:12-35), the
// first failing VoteRange. seen[k * stride], k < 16: a zeroed authority bitmap (<= 512
// authorities) for this lane.
struct LaneChecks {
  const CommitteeView& cv;
  uint32_t* seen;
  int stride;
  uint64_t me_a = 0, me_r = 0, stake = 0, epoch = 0;
  const uint8_t* me_d = nullptr;
  uint32_t inc_err = 0, vr_first = 0;
  MV_DEV void own(uint64_t a, uint64_t r, const uint8_t* d) {
    me_a = a;
    me_r = r;
    me_d = d;
  }
  MV_DEV void include(uint64_t a, uint64_t rd, const uint8_t*) {
    if (inc_err == 0) inc_err = include_code(a, rd, me_r, cv.n_auth);
    if (clock_include(a, rd, me_r, cv.n_auth)) {
      const uint32_t wd = static_cast<uint32_t>(a) >> 5, bit = 1u << (a & 31);
      const uint32_t s = seen[wd * stride];
      if (!(s & bit)) {
        seen[wd * stride] = s | bit;
        stake += cv.stakes[a];
      }
    }
  }
  MV_DEV void vote_range(uint64_t s0, uint64_t s1) {
    if (!vr_first) vr_first = vr_code(s0, s1);
  }
  MV_DEV void meta(uint64_t ep, uint64_t) { epoch = ep; }
};

// Block i = buf[o .. o + L), one lane, straight from global memory (no kernel of its own:
// ingest_block calls it for a block over its LDS window): the shared walk (bincode_walk.h) under
// the verify checks. P || sig (then 8 zero bytes) is written at stage + round_up(o, 8), which
// stays inside the block's own span because the bincode is at least |P| + 128 bytes long; writes
// happen only after the bytes they come from were read, so a malformed block never writes outside
// its span either. The buffer is readable 16 bytes past every block.
MV_DEV void ingest_lane(const uint8_t* buf, uint64_t o, uint64_t L, uint32_t i, const CommitteeView& cv,
                        const IngestOut& io, uint32_t* seen, int stride) {
  const uint64_t so = (o + 7) & ~7ull;
  BcReader r{buf + o, L, 0, true};
  PreWriter w(reinterpret_cast<uint64_t*>(io.stage + so));
  LaneChecks c{cv, seen, stride};
  const bool parsed = block_walk(r, w, c);
  uint32_t sw[16];
  uint32_t f = 0;
  if (parsed) {
    const uint8_t* sp = r.p + r.pos;
    const uint64_t plen = w.len;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint64_t v = peek8(sp + 8 * q);
      w.put(v, 8);
      sw[2 * q] = static_cast<uint32_t>(v);
      sw[2 * q + 1] = static_cast<uint32_t>(v >> 32);
    }
    w.put(0, 8);  // a zero word after P || sig
    w.flush();
    io.pre_len[i] = plen;
    f = block_facts(c.epoch == cv.epoch, c.me_a < cv.n_auth, c.me_r == 0, c.vr_first, c.stake > cv.quorum_thr,
                    c.inc_err);
  } else {
    io.pre_len[i] = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) sw[q] = 0;
  }
  io.pre_off[i] = so;
  store_block_outputs(i, f, static_cast<uint32_t>(c.me_a), sw, [&](int q) { return peek8(c.me_d + 8 * q); },
                      io.sig_out, io.claimed, io.key_idx, io.facts);
}

}  // namespace mv
