// The straight-line walk of one StatementBlock's bincode (bincode 1.3.3 defaults, data.rs:43-52;
// types.rs:93-114) that emits the signed pre-image (crypto.rs:85-128 with the CryptoHash encodings
// of crypto.rs:150-170, types.rs:661-691, 751-755), stated once for every one-lane user: the
// verify ingest's ingest_lane (ingest_lane.h) and both seal kernels (seal.hip). What parses here is
// what the library seals and what it accepts; block_codec.cpp (host) and oracle/ are the second and
// third opinions tests/test_gpu_ingest.py holds it to.
//
// Memory safety, for every caller: each offset read from the bincode passes BcReader::take against
// the block's length before it becomes an address (the caller holds off + len against the
// buffer's size first). Reads are whole aligned 8-byte words that cover a checked range, so they
// stay inside an 8-byte aligned buffer padded by 8 bytes. The walk itself stores nothing to the
// buffer: a sink or a visitor that does (the verify stage's PreWriter, seal's link) keeps to the
// block's own span and says why where it is defined.
//
// Plain C++ (no device intrinsics): with MV_DEV defined as a host function attribute the walk
// compiles for the host.
#pragma once
#include <stdint.h>

#ifndef MV_DEV
#define MV_DEV __device__ __forceinline__
#endif

namespace mv {

// 8 little-endian bytes at any address, by aligned words
MV_DEV uint64_t peek8(const uint8_t* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint64_t* w = reinterpret_cast<const uint64_t*>(a & ~static_cast<uintptr_t>(7));
  const uint32_t sh = static_cast<uint32_t>(a & 7u) * 8u;
  const uint64_t lo = w[0];
  return sh ? (lo >> sh) | (w[1] << (64u - sh)) : lo;
}

// bincode reader over one block; every read is checked against the block's length
struct BcReader {
  const uint8_t* p;
  uint64_t len, pos;
  bool ok;
  MV_DEV bool take(uint64_t k) {
    if (!ok || k > len - pos) ok = false;
    return ok;
  }
  MV_DEV uint64_t u64() {
    if (!take(8)) return 0;
    const uint64_t v = peek8(p + pos);
    pos += 8;
    return v;
  }
  MV_DEV uint32_t u32() {
    if (!take(4)) return 0;
    const uint32_t v = static_cast<uint32_t>(peek8(p + pos));
    pos += 4;
    return v;
  }
  MV_DEV uint32_t u8() {
    if (!take(1)) return 0;
    const uint32_t v = static_cast<uint32_t>(peek8(p + pos)) & 0xffu;
    pos += 1;
    return v;
  }
  // BlockReference: authority, round, digest (u64 length that must be 32, then 32 bytes)
  MV_DEV void ref(uint64_t& a, uint64_t& r, const uint8_t*& d) {
    a = u64();
    r = u64();
    const uint64_t l = u64();
    if (ok && l != 32) ok = false;
    d = p + pos;
    if (take(32)) pos += 32;
  }
};

// Bytes gathered into little-endian 64-bit words: the walk's sink. A finished word goes to
// D::word(w) (CRTP), called before nb and len move, so it sees the state ahead of the put.
template <class D>
struct ByteGather {
  uint64_t acc = 0;
  uint64_t len = 0;  // bytes put so far
  uint32_t nb = 0;   // bytes pending in acc (< 8)
  // the k low bytes of v (1 <= k <= 8; the bytes of v above them are zero)
  MV_DEV void put(uint64_t v, uint32_t k) {
    const uint64_t full = acc | (v << (8 * nb));
    const uint32_t t = nb + k;
    if (t >= 8) {
      static_cast<D*>(this)->word(full);
      acc = nb ? v >> (64 - 8 * nb) : 0ull;
      nb = t - 8;
    } else {
      acc = full;
      nb = t;
    }
    len += k;
  }
  MV_DEV void be64(uint64_t x) { put(__builtin_bswap64(x), 8); }
  MV_DEV void raw(const uint8_t* src, uint64_t k) {
    for (; k >= 8; k -= 8, src += 8) put(peek8(src), 8);
    if (k) put(peek8(src) & ((1ull << (8 * k)) - 1), static_cast<uint32_t>(k));
  }
  MV_DEV void ref(uint64_t a, uint64_t r, const uint8_t* d) {  // CryptoHash of BlockReference
    be64(a);
    be64(r);
    raw(d, 32);
  }
};
// The sink of a walk that only parses.
struct NoSink {
  MV_DEV void put(uint64_t, uint32_t) {}
  MV_DEV void be64(uint64_t) {}
  MV_DEV void raw(const uint8_t*, uint64_t) {}
  MV_DEV void ref(uint64_t, uint64_t, const uint8_t*) {}
};

// Walks the block under r and writes its pre-image P to w. Returns whether it parsed; then r.pos
// is where the 64 signature bytes lie (checked to be inside the block, not consumed). On a false
// return w holds a prefix of no use. The visitor sees what callers differ in:
//   vis.own(a, r, d)            the block's own reference (digest bytes at d)
//   vis.include(a, r, d)        one include, before its digest bytes at d are read
//   vis.vote_range(s0, s1)      one VoteRange's bounds
//   vis.meta(epoch, sig_pos)    after everything parsed; sig_pos = r.pos
// The include and statement counts are held against the bytes left (56 per include, at least
// 12 per statement) before their loops: a count past the block would fail on a later read anyway.
template <class Sink, class Visitor>
MV_DEV bool block_walk(BcReader& r, Sink& w, Visitor& vis) {
  uint64_t me_a, me_r;
  const uint8_t* me_d;
  r.ref(me_a, me_r, me_d);
  if (!r.ok) return false;
  vis.own(me_a, me_r, me_d);
  w.be64(me_a);
  w.be64(me_r);
  const uint64_t n_inc = r.u64();
  if (r.ok && n_inc > (r.len - r.pos) / 56) r.ok = false;
  for (uint64_t k = 0; r.ok && k < n_inc; k++) {
    uint64_t a, rd;
    const uint8_t* d;
    r.ref(a, rd, d);
    if (!r.ok) break;
    vis.include(a, rd, d);
    w.ref(a, rd, d);
  }
  const uint64_t n_st = r.u64();
  if (r.ok && n_st > (r.len - r.pos) / 12) r.ok = false;
  for (uint64_t k = 0; r.ok && k < n_st; k++) {
    const uint32_t tag = r.u32();
    if (!r.ok) break;
    if (tag == 0) {  // Share(Transaction): 0x00, raw bytes (no length in the pre-image)
      const uint64_t l = r.u64();
      if (!r.take(l)) break;
      w.put(0, 1);
      w.raw(r.p + r.pos, l);
      r.pos += l;
    } else if (tag == 1) {  // Vote(TransactionLocator, Vote)
      uint64_t a, rd;
      const uint8_t* d;
      r.ref(a, rd, d);
      const uint64_t lo = r.u64();
      const uint32_t vote = r.u32();
      if (!r.ok) break;
      if (vote == 0) {  // Accept
        w.put(1, 1);
        w.ref(a, rd, d);
        w.be64(lo);
      } else if (vote == 1) {  // Reject(Option<TransactionLocator>)
        const uint32_t some = r.u8();
        if (!r.ok) break;
        if (some == 0) {
          w.put(2, 1);
          w.ref(a, rd, d);
          w.be64(lo);
        } else if (some == 1) {
          uint64_t a2, rd2;
          const uint8_t* d2;
          r.ref(a2, rd2, d2);
          const uint64_t lo2 = r.u64();
          if (!r.ok) break;
          w.put(3, 1);
          w.ref(a, rd, d);
          w.be64(lo);
          w.ref(a2, rd2, d2);
          w.be64(lo2);
        } else {
          r.ok = false;
        }
      } else {
        r.ok = false;
      }
    } else if (tag == 2) {  // VoteRange(TransactionLocatorRange)
      uint64_t a, rd;
      const uint8_t* d;
      r.ref(a, rd, d);
      const uint64_t s0 = r.u64(), s1 = r.u64();
      if (!r.ok) break;
      w.put(4, 1);
      w.ref(a, rd, d);
      w.be64(s0);
      w.be64(s1);
      vis.vote_range(s0, s1);
    } else {
      r.ok = false;
    }
  }
  // meta_creation_time_ns (u128), epoch_marker (bool), epoch, signature (u64 64, then 64 bytes)
  const uint64_t tlo = r.u64(), thi = r.u64();
  const uint32_t marker = r.u8();
  if (r.ok && marker > 1) r.ok = false;
  const uint64_t ep = r.u64();
  const uint64_t sl = r.u64();
  if (r.ok && sl != 64) r.ok = false;
  if (!r.take(64)) return false;
  w.be64(thi);
  w.be64(tlo);
  w.put(marker, 1);
  w.be64(ep);
  vis.meta(ep, r.pos);
  return true;
}

}  // namespace mv
