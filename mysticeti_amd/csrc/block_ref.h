// Where a block's own BlockReference and its includes lie in bincode(Data<StatementBlock>), and
// what must hold before each load: stated once for the index kernels (index.hip, dag_store.hip) and the host
// side of mv_accept_blocks (engine_index.cpp).
//
//   own reference   bytes 0..56: authority u64, round u64, digest length u64 (32), 32 digest
//                   bytes (types.rs:49-54, 93-96; crypto.rs:322-347). process_blocks asks the core
//                   about this reference before it verifies anything (net_sync.rs:325-335), so it
//                   is read from a block that may not parse: only when len >= 56, and it counts
//                   only when the length word is 32.
//   includes        a u64 count at byte 56, then 56 bytes per include from byte 64 on, each laid
//                   out as the own reference (types.rs:97). BlockManager::add_blocks walks them
//                   after verify (block_manager.rs:75-98), so they are read only from a block that
//                   parsed; the count is bound-checked against len here all the same.
//   index key       six u64 words: authority, round and the four little-endian digest words, i.e.
//                   a reference without its length word (words 3..8 of an mv_wal_replay row).
//
// Every byte is untrusted: counts are compared as `k > room / 56`, never `64 + 56 k > len`.
#pragma once
#include <stdint.h>

namespace mv {
namespace br {

#define MV_BR_HD __host__ __device__ inline

constexpr uint64_t REF_BYTES = 56;     // a BlockReference in bincode
constexpr uint64_t LEN_WORD_OFF = 16;  // its digest length word
constexpr uint64_t DIGEST_LEN = 32;
constexpr uint64_t INC_COUNT_OFF = 56;  // the includes' count
constexpr uint64_t INC_OFF = 64;        // the first include
constexpr int KEY_WORDS = 6;

// offset of key word k (0..5) inside a bincode reference: the length word is skipped
MV_BR_HD uint64_t key_word_off(int k) { return 8 * (uint64_t)(k < 2 ? k : k + 1); }

// the own reference of a block of `len` bytes may be read
MV_BR_HD bool own_ref_readable(uint64_t len) { return len >= REF_BYTES; }

// the include count of a block of `len` bytes may be read
MV_BR_HD bool inc_count_readable(uint64_t len) { return len >= INC_OFF; }

// k includes lie inside a block of `len` bytes (len >= INC_OFF)
MV_BR_HD bool includes_inside(uint64_t len, uint64_t k) { return k <= (len - INC_OFF) / REF_BYTES; }

// offset of include j inside its block
MV_BR_HD uint64_t include_off(uint64_t j) { return INC_OFF + REF_BYTES * j; }

}  // namespace br
}  // namespace mv
