// The frame and message rules of mv_frame_messages / mv_verify_frames (include/mysti_verify.h),
// stated once for the host walk (engine.cpp) and the device walk (frames.hip).
//
//   frame_at   one step of Network::handle_read_stream (network.rs:400-447): a u32 big-endian
//              size, 0 = a ping with 8 more bytes, above MAX_SIZE = the connection is dropped
//   classify   bincode::deserialize::<NetworkMessage> (network.rs:36-46, 454-457) as far as the
//              frame's own bytes decide it: the tag, the Vec counts and lengths of tags 1 / 3
//              (data.rs:67-96), the BlockReferences of tags 2 / 4 (types.rs:49-54, a digest is a
//              u64 length of 32 + 32 bytes, crypto.rs:322-347), and RequestBlocks' limit of
//              MAXIMUM_BLOCK_REQUEST references (net_sync.rs:30, 282-285)
//
// Every byte is attacker-controlled: a load happens only after its last byte was shown to lie
// inside the frame, lengths are compared as `l > remaining` (never `q + l > end`), and a count is
// refused against remaining / (the least bytes an element takes) before any loop over it.
#pragma once
#include <stdint.h>

#include "../../include/mysti_verify.h"

namespace mv {
namespace fr {

#define MV_FR_HD __host__ __device__ inline

constexpr uint64_t MAX_SIZE = 16ull << 20;  // Network::MAX_SIZE (network.rs:216)
constexpr uint64_t PING_REST = 8;           // PING_SIZE 12 - the size word (network.rs:425, 563)
constexpr uint64_t MAX_REQUEST = 50;        // MAXIMUM_BLOCK_REQUEST (net_sync.rs:30)
constexpr uint64_t REF_BYTES = 56;          // authority, round, digest length, 32 digest bytes
constexpr uint32_t NO_TAG = 0xffffffffu;    // the row's tag word when no tag was read
constexpr uint32_t NONE = 0xffffffffu;      // bad_block / drop_msg: none
constexpr int ROW_WORDS = 8;

MV_FR_HD uint32_t ld32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
MV_FR_HD uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

enum Step : uint32_t { STEP_END, STEP_PING, STEP_FRAME, STEP_BAD_SIZE };

// The frame whose size word is at p (p <= end). STEP_END: fewer than 4 bytes, or the frame is
// not all there yet. size = the size word (STEP_FRAME: 1 .. MAX_SIZE).
MV_FR_HD Step frame_at(const uint8_t* buf, uint64_t p, uint64_t end, uint64_t& size) {
  size = 0;
  if (end - p < 4) return STEP_END;
  size = __builtin_bswap32(ld32(buf + p));
  if (size > MAX_SIZE) return STEP_BAD_SIZE;
  const uint64_t need = size ? size : PING_REST;
  if (end - p - 4 < need) return STEP_END;
  return size ? STEP_FRAME : STEP_PING;
}

struct Msg {
  uint32_t tag;     // NO_TAG when the frame is too short for one
  uint32_t status;  // MV_MSG_OK, MV_MSG_DECODE_ERROR or MV_MSG_TOO_MANY_REQUESTED
  uint32_t nblk;    // blocks of a tag 1 / 3 message that decodes, else 0
};

struct NoSink {
  MV_FR_HD void operator()(uint32_t, uint64_t, uint64_t) const {}
};

// The message in buf[body, body + size), size >= 1. sink(k, off, len) receives block k of a
// tag 1 / 3 message as it is walked (the caller discards them if the message does not decode).
template <class Sink>
MV_FR_HD Msg classify(const uint8_t* buf, uint64_t body, uint64_t size, Sink&& sink) {
  Msg m{NO_TAG, MV_MSG_DECODE_ERROR, 0};
  if (size < 4) return m;
  m.tag = ld32(buf + body);
  if (m.tag > 4) return m;
  uint64_t q = body + 4, rem = size - 4;
  if (rem < 8) return m;  // Subscribe's round, or a Vec's count
  if (m.tag == 0) {
    m.status = MV_MSG_OK;
    return m;
  }
  const uint64_t count = ld64(buf + q);
  q += 8;
  rem -= 8;
  if (m.tag == 1 || m.tag == 3) {  // Vec<Data<StatementBlock>>: u64 length + bytes each
    if (count > rem / 8) return m;
    for (uint64_t k = 0; k < count; k++) {
      if (rem < 8) return m;
      const uint64_t l = ld64(buf + q);
      q += 8;
      rem -= 8;
      if (l > rem) return m;
      sink((uint32_t)k, q, l);
      q += l;
      rem -= l;
    }
    m.nblk = (uint32_t)count;  // <= MAX_SIZE / 8
    m.status = MV_MSG_OK;
    return m;
  }
  // RequestBlocks / BlockNotFound: Vec<BlockReference>
  if (count > rem / REF_BYTES) return m;
  for (uint64_t k = 0; k < count; k++) {  // rem >= REF_BYTES * (count - k)
    if (ld64(buf + q + 16) != 32) return m;
    q += REF_BYTES;
    rem -= REF_BYTES;
  }
  m.status = (m.tag == 2 && count > MAX_REQUEST) ? MV_MSG_TOO_MANY_REQUESTED : MV_MSG_OK;
  return m;
}

MV_FR_HD void put_row(uint32_t* r, uint32_t stream, uint32_t tag, uint64_t off, uint32_t first_block, uint32_t nblk,
                      uint32_t status, uint32_t bad_status, uint32_t bad_block) {
  r[0] = stream;
  r[1] = tag;
  r[2] = (uint32_t)off;
  r[3] = (uint32_t)(off >> 32);
  r[4] = first_block;
  r[5] = nblk;
  r[6] = status | (bad_status << 8);
  r[7] = bad_block;
}

}  // namespace fr
}  // namespace mv
