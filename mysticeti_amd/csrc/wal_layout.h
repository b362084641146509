// Where WalWriter::writev puts its entries (mysticeti-core/src/wal.rs:150-188), stated once for
// mv_wal_layout (the host loop), for the kernels of mv_wal_write (wal_write.hip) and for the
// sanitizer harness (tools/wal_write_san.cpp). Plain C++: host and device compile the same text.
//
// The rule (entry_pos): an entry of `len` bytes (header + body) written at writer position p stays
// at p unless its last byte lies in another map of 2^map_bits bytes than its first; then it starts
// at that map's first byte and the bytes between are zero (wal.rs:163-172).
//
// Many entries at once. With S(i) the exclusive sum of the entry lengths, entry i stands at
// start + g + S(i), g = the gaps before it. g changes only where an entry straddles, so the
// positions are a prefix sum plus a step function of at most one step per map: cross_step finds
// the steps one after another, each by one search over S, and shift_at reads the step table.
//   state (c, g): entry c is the first of the current map run and stands at P = start + g + S(c);
//   B = the end of P's map. The first entry i >= c with start + g + S(i + 1) - 1 >= B is the next
//   that does not fit (S is strictly increasing: every entry has a header). Every entry before it
//   keeps its prefix-sum position. Entry i itself goes where entry_pos puts it: at B, with a gap,
//   when it starts before B, and where it is when it starts on B. It becomes the new c.
// An entry longer than a map would step forever: callers hand over lengths they have checked
// (entry_ok) -- mv_wal_write refuses the call before the crossings are resolved.
#pragma once
#include <stdint.h>

#ifndef MV_HD
#ifdef __HIPCC__
#define MV_HD __host__ __device__ inline
#else
#define MV_HD inline
#endif
#endif

namespace mv {
namespace wl {

constexpr uint64_t HEADER = 16;    // crc u64 | len u32 | tag u32 (combine_header, wal.rs:211-216)
constexpr uint32_t TAG_OWN = 3;    // WAL_ENTRY_OWN_BLOCK: OwnBlockData::next_entry leads the body (block_store.rs:542-549)
constexpr uint64_t OWN_HEAD = 8;
constexpr int ENTRY_WORDS = 4;     // a row of mv_wal_write: tag | payload offset | payload length | next_entry

MV_HD uint64_t map_start(uint64_t p, uint32_t map_bits) { return p & ~((1ull << map_bits) - 1); }

// the position of an entry of len bytes (1 <= len <= 2^map_bits) that the writer at p appends
MV_HD uint64_t entry_pos(uint64_t p, uint64_t len, uint32_t map_bits) {
  const uint64_t last = map_start(p + len - 1, map_bits);
  return map_start(p, map_bits) != last ? last : p;
}

// the crc'd bytes of an entry: the payload, behind the next_entry word for an own block
MV_HD uint64_t body_len(uint64_t tag, uint64_t payload_len) {
  return payload_len + ((uint32_t)tag == TAG_OWN ? OWN_HEAD : 0);
}
// what mv_wal_write refuses: a payload that leaves the buffer, a body that no map holds (wal.rs:153)
MV_HD bool entry_ok(uint64_t tag, uint64_t off, uint64_t payload_len, uint64_t buf_bytes, uint32_t map_bits) {
  if (payload_len > buf_bytes || off > buf_bytes - payload_len) return false;
  return body_len(tag, payload_len) <= (1ull << map_bits) - HEADER;
}

// One step of the crossing resolution (above). S(i), 0 <= i <= n: the exclusive sums, S(n) the
// total. find(c, T): the first i in [c, n) with S(i + 1) > T, or n. Returns false when every entry
// from c on fits the current map; else c = the entry that did not, g grown by *gap (0 when it
// starts on the boundary).
template <class Sums, class Find>
MV_HD bool cross_step(uint64_t n, uint64_t start, uint32_t map_bits, const Sums& S, const Find& find, uint64_t* c,
                      uint64_t* g, uint64_t* gap) {
  if (*c >= n) return false;
  const uint64_t P = start + *g + S(*c);
  const uint64_t B = map_start(P, map_bits) + (1ull << map_bits);
  const uint64_t i = find(*c, B - start - *g);
  if (i >= n) return false;
  const uint64_t q = start + *g + S(i);
  *gap = entry_pos(q, S(i + 1) - S(i), map_bits) - q;
  *g += *gap;
  *c = i;
  return true;
}

// the step table: cross_first[k] (ascending) = the entry in front of which gap k stands,
// cross_shift[k] = the gaps up to and including it. The shift of entry i.
MV_HD uint64_t shift_at(const uint64_t* cross_first, const uint64_t* cross_shift, uint64_t nc, uint64_t i) {
  uint64_t lo = 0, hi = nc;  // the steps below lo are at or before i, those from hi on behind it
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (cross_first[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  return lo ? cross_shift[lo - 1] : 0;
}

// The bytes of one entry in the output, all as offsets from the writer position of the call's
// first byte: [gap0, at) zero, [at, at + 16) the header, then for an own block the eight bytes of
// next_entry, then the payload from `body` to `end`.
struct Span {
  uint64_t gap0, at, body, end;
};
MV_HD Span span_of(uint64_t prev_end, uint64_t at, uint64_t tag, uint64_t payload_len) {
  const uint64_t body = at + HEADER + ((uint32_t)tag == TAG_OWN ? OWN_HEAD : 0);
  return Span{prev_end, at, body, body + payload_len};
}
// the header's two words (combine_header(crc, len, tag).to_le_bytes(): crc as u64, then len | tag << 32)
MV_HD void header_words(uint32_t crc, uint64_t tag, uint64_t payload_len, uint64_t w[2]) {
  w[0] = crc;
  w[1] = ((HEADER + body_len(tag, payload_len)) & 0xffffffffull) | ((uint64_t)(uint32_t)tag << 32);
}

}  // namespace wl
}  // namespace mv
