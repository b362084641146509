// The entry rules of mv_wal_replay (include/mysti_verify.h), stated once for the device select
// kernel (replay.hip) and any host restatement: what BlockStore::open's replay loop does with one
// WAL entry before it looks inside a block (block_store.rs:66-103).
//
//   tags       WAL_ENTRY_BLOCK 1, PAYLOAD 2, OWN_BLOCK 3, STATE 4, COMMIT 5 (block_store.rs:496-502);
//              any other tag is the loop's panic (block_store.rs:98)
//   tag 1      the payload is bincode(Data<StatementBlock>) (block_store.rs:73-74, 508)
//   tag 3      the payload is OwnBlockData's header -- next_entry, a u64 WalPosition -- and then
//              the block (block_store.rs:526-547); fewer than 8 payload bytes fail the header read
//
// Every byte is untrusted: lengths are compared as `l > remaining`, never `p + l > end`.
#pragma once
#include <stdint.h>

#include "../../include/mysti_verify.h"

namespace mv {
namespace we {

#define MV_WE_HD __host__ __device__ inline

constexpr uint32_t TAG_BLOCK = 1, TAG_PAYLOAD = 2, TAG_OWN_BLOCK = 3, TAG_STATE = 4, TAG_COMMIT = 5;
constexpr uint64_t HEADER = 16;      // crc u64 | len u32 | tag u32 (wal.rs:211-216)
constexpr uint64_t OWN_HEADER = 8;   // OwnBlockData::next_entry (block_store.rs:526-531)
constexpr uint64_t REF_BYTES = 56;   // authority, round, digest length, 32 digest bytes (types.rs:49-54)
constexpr int ROW_WORDS = 10;        // a block row of mv_wal_replay
constexpr uint64_t NONE = ~0ull;     // "no such row / entry", and next_entry of a tag-1 row

struct Entry {
  uint32_t status;   // MV_WAL_OK, MV_WAL_UNKNOWN_TAG or MV_WAL_BLOCK_DECODE
  bool block;        // the entry carries a block: image[off, off + len)
  uint64_t off, len;
};

// The entry at `pos` with `plen` payload bytes whose walk / crc status is MV_WAL_OK, in an image
// of `size` bytes. A block whose bytes are not all inside the image cannot be read in place (the
// bytes past `size` are the mapping's zero tail, of which the library keeps 16): such an entry is
// a decode failure. Its crc can only hold when the missing tail, signature bytes included, is zeros.
MV_WE_HD Entry classify(uint32_t tag, uint64_t pos, uint64_t plen, uint64_t size) {
  Entry e{MV_WAL_OK, false, 0, 0};
  if (tag < TAG_BLOCK || tag > TAG_COMMIT) {
    e.status = MV_WAL_UNKNOWN_TAG;
    return e;
  }
  if (tag != TAG_BLOCK && tag != TAG_OWN_BLOCK) return e;
  const uint64_t skip = tag == TAG_OWN_BLOCK ? OWN_HEADER : 0;
  e.status = MV_WAL_BLOCK_DECODE;
  if (plen < skip) return e;
  if (pos > size || HEADER > size - pos || plen > size - pos - HEADER) return e;
  e.status = MV_WAL_OK;
  e.block = true;
  e.off = pos + HEADER + skip;
  e.len = plen - skip;
  return e;
}

}  // namespace we
}  // namespace mv
