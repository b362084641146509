// The rules of mv_encode_blocks, stated once for the kernels (encode.hip) and for the host harness
// that runs them under the sanitizers (tools/encode_san.cpp): the payload check, the head checks and
// the length formula, and the piece table of a block -- the function from a destination byte offset
// to its source. The inverse of bincode_walk.h: what is written here parses there.
//
// A block of k includes whose payloads have bodies of b_0 .. b_{P-1} bytes (a body is a payload
// without its count word), B their sum, S_j the sum of the first j:
//
//   piece           destination bytes            source
//   fixed head      [0, 64)                      head words 0, 1; 32; four zero words; k
//   include rows    [64, 64 + 56 k)              row r at 64 + 56 r: words 0, 1 of includes row
//                                                first + r; 32; its words 2..5
//   count word      [64 + 56 k, 72 + 56 k)       the sum of the payloads' counts
//   body j          [72 + 56 k + S_j, .. + b_j)  payload j's bytes from 8 on
//   tail            [72 + 56 k + B, .. + 97)     head words 2, 3; the marker byte; head word 4; 64;
//                                                64 zero bytes
//   padding         up to the next multiple of 8 zero
//
// Everything up to the first body is made of whole words on word boundaries; a body may have any
// length, so every piece behind the first non-empty body starts at any byte. dest_word assembles one
// aligned destination word from the pieces it straddles, at most eight of them.
//
// Memory safety: a head's runs are held against m and p (run_inside) before an index is formed, a
// payload's span against the buffer before a byte of it is read, and BlockSrc checks every index
// and offset again where it becomes an address: a failed check calls Err and yields zero bytes.
// Payload bytes are read by peek8, whole aligned words that cover a checked range: the buffer is
// 8-byte aligned and readable up to the next multiple of 8 past its size plus 8.
//
// Plain C++ (no device intrinsics): with MV_DEV and MV_VT_DEV defined as host function attributes it
// compiles for the host.
#pragma once
#include <stdint.h>

#include "../../include/mysti_verify.h"
#include "bincode_walk.h"
#include "votes_walk.h"

namespace mv::en {

constexpr uint64_t HEAD_WORDS = 10, REF_WORDS = 6;
constexpr uint64_t HEAD_BYTES = 64, REF_BYTES = 56, TAIL_BYTES = 97;
constexpr uint64_t FIXED_BYTES = HEAD_BYTES + 8 + TAIL_BYTES;  // a block without includes and statements
static_assert(FIXED_BYTES == 169, "the length formula of include/mysti_verify.h");
enum HeadWord { H_AUTH = 0, H_ROUND, H_TIME_LO, H_TIME_HI, H_EPOCH, H_MARKER, H_INC0, H_NINC, H_PAY0, H_NPAY };

MV_DEV uint64_t round_up8(uint64_t x) { return (x + 7) & ~7ull; }
MV_DEV uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
// the run [first, first + count) lies inside [0, size): no sum is formed that could wrap
MV_DEV bool run_inside(uint64_t first, uint64_t count, uint64_t size) { return first <= size && count <= size - first; }

// the statement walk's visitor that does nothing
struct NoVotes {
  MV_DEV void share(uint64_t) {}
  MV_DEV void vote(uint64_t, const uint64_t*, uint64_t) {}
  MV_DEV void reject(uint64_t) {}
  MV_DEV void range(uint64_t, const uint64_t*, uint64_t, uint64_t) {}
};

// The payload check: buf[off, off + len) lies inside the buffer's `bytes`, passes the statement
// walk, and the walk ends on its last byte. *count = its statements, *body = len - 8.
MV_VT_DEV bool check_payload(const uint8_t* buf, uint64_t bytes, uint64_t off, uint64_t len, uint64_t* count,
                             uint64_t* body) {
  *count = 0, *body = 0;
  if (!run_inside(off, len, bytes)) return false;
  BcReader r{buf + off, len, 0, true};
  NoVotes f;
  uint64_t c = 0;
  if (!mv::ix::walk_statements(r, f, &c) || r.pos != len) return false;
  *count = c, *body = len - 8;
  return true;
}

MV_DEV bool head_ok(const uint64_t* h, uint64_t m, uint64_t p) {
  return h[H_MARKER] <= 1 && run_inside(h[H_INC0], h[H_NINC], m) && run_inside(h[H_PAY0], h[H_NPAY], p);
}
// 169 + 56 k + body, all ones when that is more than any block may have
MV_DEV uint64_t block_len(uint64_t k, uint64_t body) {
  if (k > MV_ENCODE_MAX_LEN / REF_BYTES) return ~0ull;
  return sat_add(FIXED_BYTES + REF_BYTES * k, body);
}

// A block's verdict from its head and the per-payload results of check_payload (p entries each), in
// the order of the header: head, payloads, length. *len = its length, *count = its statements (both
// 0 unless MV_ENCODE_OK).
MV_DEV uint32_t size_block(const uint64_t* h, uint64_t m, uint64_t p, const uint8_t* pay_ok, const uint64_t* pay_body,
                           const uint64_t* pay_count, uint64_t* len, uint64_t* count) {
  *len = 0, *count = 0;
  if (!head_ok(h, m, p)) return MV_ENCODE_BAD_HEAD;
  uint64_t body = 0, sts = 0;
  const uint64_t j0 = h[H_PAY0], j1 = j0 + h[H_NPAY];  // (inside [0, p]: head_ok)
  for (uint64_t j = j0; j < j1; j++) {
    if (!pay_ok[j]) return MV_ENCODE_BAD_PAYLOAD;
    body = sat_add(body, pay_body[j]);
    sts += pay_count[j];  // (at most body / 12: it wraps only where body saturates)
  }
  const uint64_t l = block_len(h[H_NINC], body);
  if (l > MV_ENCODE_MAX_LEN) return MV_ENCODE_TOO_LONG;
  *len = l, *count = sts;
  return MV_ENCODE_OK;
}

// The inputs of a call.
struct Inputs {
  const uint64_t* heads;
  const uint64_t* includes;
  uint64_t m;
  const uint8_t* payload_buf;
  uint64_t payload_bytes;
  const uint64_t *payload_off, *payload_len;
  uint64_t p;
};

// A block's shape: what the piece table needs beyond the inputs.
struct Shape {
  uint64_t k, inc0, pay0, np;
  uint64_t count;  // the statements of all its payloads
  uint64_t body;   // B
  uint64_t len;    // 169 + 56 k + B
  MV_DEV uint64_t body0() const { return HEAD_BYTES + REF_BYTES * k + 8; }
  MV_DEV uint64_t tail0() const { return body0() + body; }
};

// The shape of block i, whose length the size pass gave as len and whose statements as count, from
// its head and the scan of the bodies (pre: p + 1 entries, modulo 2^64). False when the head fails
// its checks again or the two passes disagree about the length.
MV_DEV bool shape_of(const Inputs& in, uint64_t i, const uint64_t* pre, uint64_t count, uint64_t len, Shape* sh) {
  const uint64_t* h = in.heads + HEAD_WORDS * i;
  if (!head_ok(h, in.m, in.p)) return false;
  *sh = Shape{h[H_NINC], h[H_INC0], h[H_PAY0], h[H_NPAY], count, 0, len};
  sh->body = pre[sh->pay0 + sh->np] - pre[sh->pay0];
  return block_len(sh->k, sh->body) == len;
}
// the block's padded span lies inside the cap bytes of the output, on a word boundary
MV_DEV bool span_ok(uint64_t off, uint64_t len, uint64_t cap) { return !(off & 7) && run_inside(off, round_up8(len), cap); }

// up to 8 bytes of a piece from some position on: the bytes (low first) and how many of them
// belong to the piece (1..8)
struct Run {
  uint64_t v;
  uint32_t n;
};
MV_DEV uint64_t low_bytes(uint64_t v, uint32_t n) { return n >= 8 ? v : v & ((1ull << (8 * n)) - 1); }
// the bytes of a `width`-byte little-endian field holding v, from byte `at` of it on
MV_DEV Run field_run(uint64_t v, uint32_t width, uint32_t at) { return Run{v >> (8 * at), width - at}; }

// The sources of block i, every access checked. Pre: pre(j) = S_j for 0 <= j <= np (the kernel
// keeps them in LDS, the harness in a vector). Err: called for a failed check.
template <class Pre, class Err>
struct BlockSrc {
  const Inputs& in;
  uint64_t i;
  Shape sh;
  Pre pre;
  Err err;

  MV_DEV uint64_t head(uint32_t w) const { return in.heads[HEAD_WORDS * i + w]; }
  MV_DEV uint64_t inc(uint64_t row, uint32_t w) const {
    if (row >= sh.k || !run_inside(sh.inc0, row + 1, in.m)) {
      err();
      return 0;
    }
    return in.includes[REF_WORDS * (sh.inc0 + row) + w];
  }
  // the payload whose body holds body byte q (q < B): the last j with S_j <= q, which skips the empty
  // bodies that start at q too
  MV_DEV uint64_t payload_of(uint64_t q) const {
    uint64_t lo = 0, hi = sh.np;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (pre(mid) <= q) lo = mid;
      else hi = mid;
    }
    return lo;
  }
  // the bytes of the bodies from body byte q on, up to the end of the body that holds q
  MV_DEV Run body_run(uint64_t q) const {
    const uint64_t j = payload_of(q);
    const uint64_t s0 = pre(j), s1 = pre(j + 1);
    if (j >= sh.np || !run_inside(sh.pay0, j + 1, in.p) || q < s0 || q >= s1) {
      err();
      return Run{0, 1};
    }
    const uint64_t off = in.payload_off[sh.pay0 + j], len = in.payload_len[sh.pay0 + j];
    const uint64_t at = 8 + (q - s0), left = s1 - q;  // the byte inside the payload, the bytes behind it
    const uint32_t n = left < 8 ? (uint32_t)left : 8u;
    if (!run_inside(off, len, in.payload_bytes) || !run_inside(at, n, len)) {
      err();
      return Run{0, 1};
    }
    return Run{low_bytes(peek8(in.payload_buf + off + at), n), n};
  }
  // the bytes of the block from byte pos on (pos < len), up to the end of the field that holds pos
  MV_DEV Run run_at(uint64_t pos) const {
    const uint64_t b0 = sh.body0(), t0 = sh.tail0();
    if (pos < b0) {  // whole words on word boundaries
      const uint64_t w = pos / 8;
      const uint32_t at = (uint32_t)(pos & 7);
      uint64_t v;
      if (w < 8) {
        v = w == 0 ? head(H_AUTH) : w == 1 ? head(H_ROUND) : w == 2 ? 32 : w == 7 ? sh.k : 0;
      } else if (w < 8 + 7 * sh.k) {
        const uint64_t row = (w - 8) / 7;
        const uint32_t f = (uint32_t)((w - 8) % 7);
        v = f == 2 ? 32 : inc(row, f < 2 ? f : f - 1);
      } else {
        v = sh.count;
      }
      return field_run(v, 8, at);
    }
    if (pos < t0) return body_run(pos - b0);
    const uint64_t t = pos - t0;
    if (t < 8) return field_run(head(H_TIME_LO), 8, (uint32_t)t);
    if (t < 16) return field_run(head(H_TIME_HI), 8, (uint32_t)(t - 8));
    if (t < 17) return field_run(head(H_MARKER), 1, 0);
    if (t < 25) return field_run(head(H_EPOCH), 8, (uint32_t)(t - 17));
    if (t < 33) return field_run(64, 8, (uint32_t)(t - 25));
    return Run{0, 8};  // the signature's placeholder (the loop below stops at len)
  }
  // The destination word at byte o of the block (o a multiple of 8, o < round_up8(len)): the
  // pieces it straddles, the bytes from len on zero.
  MV_DEV uint64_t dest_word(uint64_t o) const {
    uint64_t word = 0;
    uint32_t have = 0;
    while (have < 8 && o + have < sh.len) {
      const Run r = run_at(o + have);
      uint32_t n = r.n < 8 - have ? r.n : 8 - have;
      const uint64_t left = sh.len - (o + have);
      if (left < n) n = (uint32_t)left;
      word |= low_bytes(r.v, n) << (8 * have);
      have += n;
    }
    return word;
  }
};

}  // namespace mv::en
