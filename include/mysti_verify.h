/* mysti_verify.h — C ABI of the MI355X StatementBlock verification engine.
 *
 * Drop-in boundary for the per-block crypto of hrubaanna/mysticeti
 * (reference @ 2025-02-04). Each entry point names the reference interface it
 * replaces (paths relative to the reference repo):
 *
 *   mv_blake2b256          BlockHasher = blake2::Blake2b<U32> (mysticeti-core/src/crypto.rs:34),
 *                          as used by BlockDigest::new (crypto.rs:38-61)
 *   mv_ed25519_verify      PublicKey::verify_block -> ed25519_consensus::VerificationKey::verify
 *                          (crypto.rs:174-189; ZIP-215 semantics of ed25519-consensus 2.1.0)
 *   mv_ed25519_sign        Signer::sign_block -> ed25519_consensus::SigningKey::sign
 *                          (crypto.rs:199-223; RFC 8032)
 *   mv_set_committee       Committee::get_public_key / stake (committee.rs:56-87); the
 *                          VerificationKey decode that happens once per authority
 *   mv_verify_blocks       the loop `for block in blocks { block.verify(&committee) }` of
 *                          NetworkSyncer::process_blocks (net_sync.rs:331-375) over
 *                          StatementBlock::verify (types.rs:315-376), on Data<StatementBlock>
 *                          bincode bytes (data.rs:43-52)
 *   mv_dev_ed25519_verify_batch
 *                          ed25519_consensus::batch::Verifier (the ZIP-215 batch rule, which agrees
 *                          with VerificationKey::verify) over a whole batch, with an exact
 *                          per-signature fallback: per-item verdicts equal mv_ed25519_verify's
 *   mv_dev_*               the same computations on device-resident buffers (HBM in, HBM out)
 *   mv_crc32               crc32fast::hash (crc32fast 1.3.2, Cargo.lock:777), as the WAL uses it
 *                          (mysticeti-core/src/wal.rs:173-177, :250)
 *   mv_wal_verify          WalReader::iter_until + WalIterator::next over WalReader::try_read
 *                          (wal.rs:226-346): the entry walk and crc check of the WAL replay in
 *                          BlockStore::open (block_store.rs:66)
 *   mv_wal_replay          the replay loop of BlockStore::open on top of that walk (block_store.rs:50-116):
 *                          the tag match (:71-99), the decode of WAL_ENTRY_BLOCK / WAL_ENTRY_OWN_BLOCK
 *                          entries (:73-74, 83-84, 526-540), each block's BlockReference for add_unloaded,
 *                          highest_round and last_seen_by_authority (:398-404, 424-432), and the positions
 *                          RecoveredStateBuilder wants (state.rs:39-59); also StatementBlock::verify of
 *                          every block, which the reference's replay skips
 *   mv_wal_recover         that replay, and the replayed blocks as stored blocks with their edges in
 *                          the DAG store: what BlockStore::open with add_unloaded (block_store.rs:398-404)
 *                          leaves for BaseCommitter to read after a restart
 *   mv_wal_layout          WalWriter::writev position arithmetic (wal.rs:150-188), host only
 *   mv_wal_write           WalWriter::writev itself for n entries (wal.rs:150-188, 211-216): positions, crc32
 *                          headers, padding and bodies, as BlockWriter::insert_block and
 *                          OwnBlockData::write_to_wal use it (block_store.rs:504-518, 542-549)
 *   mv_frame_blocks        the block byte strings of received NetworkMessage frames
 *                          (Network::handle_read_stream, network.rs:400-447), host only
 *   mv_verify_frames       what a connection does with its received bytes, per message: the frame
 *                          reads of handle_read_stream (network.rs:400-447), the decode of each
 *                          NetworkMessage (network.rs:454-457, data.rs:83-96) and
 *                          NetworkSyncer::process_blocks (net_sync.rs:314-383), whose first
 *                          rejected block ends the message and the connection
 *   mv_frame_messages      the same walk on the host for one stream, without the block verdicts
 *   mv_index_*             the set of BlockReferences the core answers from: BlockManager::exists_or_pending
 *                          (block_manager.rs:142-144) and BlockManager::missing (:26, 90-97, 138-140), kept in
 *                          device memory
 *   mv_accept_blocks       NetworkSyncer::process_blocks with its `processed` query and skip
 *                          (net_sync.rs:325-336, core_thread/spawned.rs:140-150) ahead of verify, and after it the
 *                          include lookups of BlockManager::add_blocks (block_manager.rs:48-136) whose result the
 *                          syncer requests from peers (net_sync.rs:388-398)
 *   mv_connect_blocks      mv_accept_blocks and the suspend / unlock cascade of add_blocks (block_manager.rs:102-131)
 *                          over a store of suspended blocks in device memory: the blocks the core may process,
 *                          in a causal order
 *   mv_dag_*, mv_decide_leaders   the edges of the blocks mv_connect_blocks stored, kept in device memory, and
 *                          BaseCommitter::try_direct_decide (consensus/base_committer.rs:323-357) over them at
 *                          the production wave length 3, which UniversalCommitter::try_commit
 *                          (consensus/universal_committer.rs:30-90) runs for every undecided leader after
 *                          every add_blocks
 *   mv_commit_leaders      try_commit itself: the direct rule, try_indirect_decide (:294-318) over
 *                          BlockStore::linked_to_round (block_store.rs:306-327), and the decided prefix
 *   mv_linearize           Linearizer::handle_commit (consensus/linearizer.rs:125-166): each committed leader's
 *                          sub-DAG in the reference's own order, with the committed marks and last_height
 *   mv_propose_*           what Core does between add_blocks and new_with_signer: the threshold clock
 *                          (threshold_clock.rs:58-89), the `pending` queue (core.rs:197-198, 223-224) and the
 *                          include choice of Core::try_new_block (core.rs:232-278), with the own block's record
 *   mv_seal_blocks         StatementBlock::new_with_signer (types.rs:155-218) on blocks that are bincode
 *                          already: Signer::sign_block (crypto.rs:199-223) over the digest of the signed
 *                          pre-image (crypto.rs:85-128) and BlockDigest::new (crypto.rs:38-61), written
 *                          into the block's own bytes; with MV_SEAL_LINK a whole DAG, round by round
 *
 * Conventions
 *   - The caller owns every buffer passed in and out; they must stay valid for the call.
 *     The library copies host inputs into its own pinned staging and device memory.
 *   - Return value: MV_OK (0) or a negative MV_E_* code; mv_last_error() gives text.
 *     Per-item verdicts go to caller arrays: a rejected signature is not an error.
 *   - Host-buffer calls are synchronous and thread-safe on one context. mv_verify_blocks callers
 *     are coalesced (a submission queue merges concurrent calls into shared device passes);
 *     the other host-buffer calls take the context in turn.
 *   - A context spans the devices in mv_config.device_mask; host-buffer calls shard
 *     their items across them (no collective: each device returns its slice of verdicts).
 */
#ifndef MYSTI_VERIFY_H
#define MYSTI_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mv_ctx mv_ctx;
typedef int32_t mv_status;

#define MV_OK 0
#define MV_E_INVALID_ARG (-1)
#define MV_E_HIP (-2)
#define MV_E_NO_DEVICE (-3)
#define MV_E_NO_COMMITTEE (-4)
#define MV_E_ALLOC (-5)
#define MV_E_INDEX_FULL (-6) /* a device-buffer index call: the entries it could add do not fit the reserved index */

/* per-signature verdicts (ed25519_consensus::Error mapping) */
#define MV_SIG_OK 0
#define MV_SIG_INVALID 1       /* Error::InvalidSignature */
#define MV_SIG_MALFORMED_KEY 2 /* Error::MalformedPublicKey (A does not decode) */

/* per-block verdicts, in the error order of StatementBlock::verify (types.rs:315-376) */
#define MV_BLOCK_OK 0
#define MV_BLOCK_PARSE_ERROR 1             /* bincode::deserialize failed (data.rs:43-52) */
#define MV_BLOCK_DIGEST_MISMATCH 2         /* "Digest does not match" types.rs:327-332 */
#define MV_BLOCK_EPOCH_MISMATCH 3          /* types.rs:333-338 */
#define MV_BLOCK_UNKNOWN_AUTHOR 4          /* types.rs:339-342 */
#define MV_BLOCK_GENESIS 5                 /* types.rs:343-345 */
#define MV_BLOCK_SIG_INVALID 6             /* types.rs:346-348 */
#define MV_BLOCK_INCLUDE_UNKNOWN_AUTHORITY 7 /* types.rs:350-355 */
#define MV_BLOCK_INCLUDE_ROUND 8           /* types.rs:356-361 */
#define MV_BLOCK_VOTE_RANGE 9              /* first failing VoteRange (types.rs:363-370): end < start, */
                                           /* "offset_end_exclusive must be greater or equal ..." :441-446 */
#define MV_BLOCK_THRESHOLD_CLOCK 10        /* types.rs:371-374, threshold_clock.rs:12-35 */
#define MV_BLOCK_VOTE_RANGE_TOO_LONG 11    /* end - start >= 2^20, "Include is too large ..." :447-453 */
#define MV_BLOCK_VOTE_RANGE_END_TOO_LARGE 12 /* end >= 2^20, "offset_end_exclusive is too large ..." :454-458 */

/* per-entry WAL verdicts (WalReader::try_read, wal.rs:233-261; the reference panics on all but OK) */
#define MV_WAL_OK 0
#define MV_WAL_CRC_MISMATCH 1     /* "Crc mismatch, expected .., found .." wal.rs:250-257 */
#define MV_WAL_NONZERO_CRC_LEN0 2 /* "Non-zero crc at len 0" wal.rs:240-247 */
#define MV_WAL_BAD_LENGTH 3       /* len < 16 or the entry runs past its map: Bytes::slice panics, wal.rs:249 */
/* ... and of the replay loop of BlockStore::open, produced by mv_wal_replay / mv_dev_wal_replay only
 * (each is a panic of the reference) */
#define MV_WAL_UNKNOWN_TAG 4       /* tag not in 1..5: "Unknown wal tag", block_store.rs:98 */
#define MV_WAL_BLOCK_DECODE 5      /* tag 1 whose payload does not deserialize (block_store.rs:73-74); tag 3 with */
                                   /* fewer than 8 payload bytes (:531) or whose block, from byte 8 on, does not (:84, 534) */
#define MV_WAL_UNKNOWN_AUTHORITY 6 /* the block decodes, its authority >= the committee size: the expect in */
                                   /* update_last_seen_by_authority, block_store.rs:424-428 */

/* per-message verdicts of mv_verify_frames / mv_frame_messages: what the reference does with one
 * received NetworkMessage (network.rs:400-457, net_sync.rs:272-383) */
#define MV_MSG_OK 0                 /* decodes, and every block of it is MV_BLOCK_OK (also: no blocks) */
#define MV_MSG_DECODE_ERROR 1       /* bincode::deserialize::<NetworkMessage> fails, network.rs:454-457 */
#define MV_MSG_BLOCK_REJECTED 2     /* process_blocks returns Err at its first rejected block, net_sync.rs:352-361 */
#define MV_MSG_TOO_MANY_REQUESTED 3 /* RequestBlocks above MAXIMUM_BLOCK_REQUEST = 50, net_sync.rs:30, 282-285 */
#define MV_MSG_NOT_REACHED 4        /* after the message that ended the connection: never processed */
#define MV_MSG_BAD_SIZE 5           /* frame size above MAX_SIZE = 16 MiB, network.rs:216, 419-422 */

/* states of a BlockReference in the index (mv_index_*). State only rises: the reference never removes
 * from these sets (unload_below_round only unloads block bodies). */
#define MV_REF_ABSENT 0 /* no entry */
#define MV_REF_WANTED 1 /* an accepted block includes it and it has not arrived: a key of block_references_waiting
                           that is not pending, i.e. BlockManager::missing (block_manager.rs:90-97) */
#define MV_REF_HAVE 2   /* stored or pending: BlockManager::exists_or_pending (block_manager.rs:142-144) */
#define MV_REF_STORED 3 /* in the store: the block and its whole causal history have been accepted
                           (BlockStore::block_exists). Only mv_connect_blocks and a caller's seeding produce it;
                           every call that asks for HAVE means HAVE or STORED */

/* per-block outcome of mv_accept_blocks */
#define MV_ACC_REJECTED 0 /* its own MV_BLOCK_* is not OK */
#define MV_ACC_NEW 1      /* accepted, first with its reference: add_blocks goes on with it */
#define MV_ACC_KNOWN 2    /* processed before: skipped ahead of verify (net_sync.rs:333-336) */
#define MV_ACC_DUP 3      /* accepted, but a block of a lower index has the same reference (block_manager.rs:68-72) */
#define MV_ACC_DROPPED 4  /* OK itself, but a block of its group was rejected: process_blocks returned before
                             add_blocks (net_sync.rs:352-361) */
#define MV_ACC_SUSPENDED 5 /* mv_connect_blocks only: accepted as MV_ACC_NEW, but an include is not stored yet:
                              the block waits in blocks_pending (block_manager.rs:102-110) */

/* mv_config.flags */
#define MV_FLAG_NO_BATCH 1u /* host-buffer verify: never use the batch (random linear combination) path */
#define MV_FLAG_NO_COMB 2u  /* committee-key verifies: never use the per-key comb tables (ladder per signature) */
#define MV_FLAG_HOST_PARSE 4u /* mv_verify_blocks: parse the bincode on the host (block_codec.cpp), not on the GPU */
#define MV_FLAG_NO_ONLINE 8u  /* mv_verify_blocks: never use the resident online service (every call goes
                                 through the submission queue and launches its own kernels) */

/* Host-buffer verify calls of at least this many signatures per device take the batch path
 * (one combined equation + exact fallback); smaller ones verify every signature alone. */
#define MV_BATCH_MIN 4096u

typedef struct mv_config {
  uint32_t device_mask; /* bit i = use HIP device i; 0 = device 0 only */
  uint32_t max_batch;   /* items per device launch chunk; 0 = default (1<<20) */
  uint32_t flags;       /* MV_FLAG_* */
  uint32_t shards_per_device; /* 0/1 = one; k > 1: k logical shards (stream + buffers each) per device,
                                 host-buffer calls shard across them exactly as across GPUs */
} mv_config;

mv_status mv_create(const mv_config* cfg, mv_ctx** out);
void mv_destroy(mv_ctx* ctx);
const char* mv_last_error(const mv_ctx* ctx);
/* library version string, e.g. "mysti_verify 0.1 gfx950" */
const char* mv_version(void);

/* Committee: n authority keys (32-byte encodings) and stakes, committee epoch.
 * key_ok[i] (optional) receives 1 if key i decodes (VerificationKey::try_from).
 * MV_E_INVALID_ARG (the committee in force stays) when n is 0 or above 512, or when the total
 * stake or twice the total does not fit in 64 bits: Committee::new refuses an overflowing total
 * (committee.rs:50-54), and the quorum threshold is 2 * total / 3 (committee.rs:56-57). */
mv_status mv_set_committee(mv_ctx* ctx, const uint8_t* pks /* n x 32 */, const uint64_t* stakes, uint32_t n,
                           uint64_t epoch, uint8_t* key_ok /* n, may be NULL */);

/* Blake2b-256 of n byte strings buf[off[i] .. off[i]+len[i]) -> out[i] (32 B each). */
mv_status mv_blake2b256(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                        uint8_t* out /* n x 32 */);

/* ZIP-215 ed25519 verification of n signatures over 32-byte messages.
 * Keys: pk[i] if key_idx == NULL, else committee key key_idx[i] (pk must be NULL). */
mv_status mv_ed25519_verify(mv_ctx* ctx, const uint8_t* msg /* n x 32 */, const uint8_t* sig /* n x 64 */,
                            const uint8_t* pk /* n x 32 or NULL */, const uint32_t* key_idx /* n or NULL */,
                            uint32_t n, uint8_t* status /* n, MV_SIG_* */);

/* Page-locked host memory for verify inputs (hipHostMalloc, portable across the context's
 * devices). mv_ed25519_verify on inputs that are pinned (these, or any hipHostMalloc /
 * hipHostRegister memory) streams them in chunks whose H2D copies run beside the verification
 * of the previous chunk, instead of one pageable copy before the whole batch. Free with
 * mv_host_free. The Rust caller would receive network payloads into such buffers. */
mv_status mv_host_alloc(mv_ctx* ctx, uint64_t bytes, void** out);
void mv_host_free(mv_ctx* ctx, void* p);

/* RFC 8032 signing of n 32-byte messages with n 32-byte seeds -> pk (n x 32), sig (n x 64). */
mv_status mv_ed25519_sign(mv_ctx* ctx, const uint8_t* seed, const uint8_t* msg, uint32_t n, uint8_t* pk,
                          uint8_t* sig);

/* StatementBlock::verify on n bincode-serialized blocks buf[off[i] .. off[i]+len[i]).
 * status[i] = MV_BLOCK_*; msg_digest[i] = Blake2b-256(pre-image) (the signed message),
 * block_digest[i] = Blake2b-256(pre-image || signature); either digest array may be NULL.
 * Requires mv_set_committee. Concurrent callers are coalesced: a call joins a submission
 * queue, and a caller that finds no device pass running takes every queued call into one
 * pass (the online path: n - 1 peer tasks each with a block or two share a GPU round trip).
 * Several devices: the merged blocks are split into contiguous shards of about equal bytes.
 * Parameter order: status comes before the two (optional) digest arrays, unlike the draft in
 * SURVEY.md 8(b), so that the required outputs precede the NULL-able ones; `len` is u64 (blocks
 * are not bounded by 4 GiB in the type, and off/len share one type). */
mv_status mv_verify_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                           uint8_t* status, uint8_t* msg_digest, uint8_t* block_digest);

/* Submission-queue counters: mv_verify_blocks calls, and device passes that served them. */
mv_status mv_queue_stats(mv_ctx* ctx, uint64_t* calls, uint64_t* passes);

/* The resident online service (replaces the per-call device pass for the one-task-per-peer
 * traffic of NetworkSyncer, net_sync.rs:214-221 / synchronizer.rs:146-164): mv_verify_blocks
 * calls of <= 64 blocks and <= 128 KB of bincode, every block inside the device ingest's 10-KB
 * window (short and config-4-shape long blocks alike; MV_ONLINE_LONG=0 restricts the service to
 * calls averaging < MV_COMB_SPLIT_BYTES per block), are posted to a ring in page-locked memory
 * that a kernel resident on a highest-priority stream (a hardware queue of its own) polls; the
 * caller's thread spins on its
 * request's done word (no launch, no event, no wake-up per call). The kernel exits after
 * MV_ONLINE_IDLE_US (default 10,000) without work and is relaunched by the next call; calls it
 * does not take (more blocks or bytes, a block past the window, MV_FLAG_NO_ONLINE, MV_ONLINE=0)
 * go through the submission queue, and so does every call after the service has failed.
 * Verdicts and digests are those of the queue path. Counters: requests served by the service
 * and kernel launches it needed, summed over the context's devices. */
mv_status mv_online_stats(mv_ctx* ctx, uint64_t* requests, uint64_t* launches);

/* Host-only helper (no device needed): the shard plan of the multi-device paths -- cut[0..parts]
 * splits items [0, n) into contiguous shards of about equal total weight (block calls weigh a
 * block by its bincode bytes + 64). */
mv_status mv_shard_plan(const uint64_t* weights, uint64_t n, uint32_t parts, uint64_t* cut /* parts + 1 */);

/* Host-only helper (no device needed): the signed pre-image of one bincode block
 * (BlockDigest::digest_without_signature, crypto.rs:85-128). Returns the pre-image
 * length, or -1 if the bytes do not deserialize. `out` may be NULL to query the length. */
int64_t mv_block_preimage(const uint8_t* bincode, uint64_t len, uint8_t* out, uint64_t cap);

/* crc32fast::hash (CRC-32/ISO-HDLC) of n byte strings buf[off[i] .. off[i]+len[i]) -> out[i]. */
mv_status mv_crc32(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                   uint32_t* out /* n */);

/* WAL replay check: iterates the WAL image wal[0 .. size) as WalReader::iter_until does up to the
 * writer position end_pos (maps of 2^map_bits bytes: 24 in production, 16 under cfg(test),
 * wal.rs:95-103; 8 <= map_bits <= 30), checking every entry's crc32. Entries come out in
 * iteration order: pos[i] (WalPosition.start), tag[i], len[i] (payload bytes), status[i]
 * (MV_WAL_*). The iteration stops after the first entry whose status is not MV_WAL_OK (where
 * the reference panics). *count = the number of entries; only the first `cap` are written.
 * Bytes at or past `size` read as zero (the mapping's tail past the end of the file). */
mv_status mv_wal_verify(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                        uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap,
                        uint64_t* count);

/* WAL replay up to the block-store index: what BlockStore::open does with a WAL (block_store.rs:50-116),
 * with the blocks verified. The walk and the crc check are mv_wal_verify's (same arguments, same
 * pos / tag / len / status / count, same iteration order, the first `cap` entries written); the
 * image stays in device memory and the rest of the replay loop runs on it there:
 *
 * Entries. Where mv_wal_verify says MV_WAL_OK, the replay loop's own panics become the entry's
 * status: MV_WAL_UNKNOWN_TAG (tag not in 1..5), MV_WAL_BLOCK_DECODE (a tag-1 payload, or a tag-3
 * payload from byte 8 on, that is MV_BLOCK_PARSE_ERROR; a tag-3 payload under 8 bytes; also a
 * tag-1 / tag-3 payload that reaches past `size`, whose zero tail the library does not read),
 * MV_WAL_UNKNOWN_AUTHORITY (the block decodes but its authority >= the committee size; the decode
 * is checked first). The list ends with the first entry, in iteration order, whose status is not
 * MV_WAL_OK, whatever made it so; *count includes that entry.
 * The payloads of tags 2, 4 and 5 (payload, state, commit) are not decoded: RecoveredStateBuilder
 * decodes them on the host (state.rs:39-59), from pos / len.
 *
 * Block rows. One row of 10 uint64_t words per tag-1 / tag-3 entry that is MV_WAL_OK after all of
 * the above, in iteration order (the failing entry and everything after it get none):
 *   [0] entry index   [1] offset of the block's bincode in the image (pos + 16, + 8 for tag 3)
 *   [2] its length    [3] authority   [4] round
 *   [5..8] the 32 digest bytes as stored (four little-endian words): the claimed digest, the index
 *          key of add_unloaded
 *   [9] OwnBlockData::next_entry of a tag-3 entry (the payload's first u64), else UINT64_MAX
 * blk_status[r] (optional) = the MV_BLOCK_* of StatementBlock::verify on row r's block. A block
 * that parses but is rejected (digest mismatch, bad signature, threshold clock, ...) does not end
 * the replay -- the reference does not verify here -- the status is information for the caller.
 * *n_blocks = the number of rows; the first cap_blocks are written.
 *
 * Summary, over the rows kept: summary[0] = highest_round (0 without rows); summary[1] = the row
 * index of the last tag-3 row, or UINT64_MAX (last_own_block, state.rs:49-54); summary[2] = the entry
 * index of the last MV_WAL_OK tag-4 entry, or UINT64_MAX (it clears unprocessed_blocks, state.rs:56-59);
 * last_seen[a] (committee size words) = the largest round of authority a's rows, 0 if none
 * (block_store.rs:57, 424-432).
 * Requires mv_set_committee (MV_E_NO_COMMITTEE otherwise), as BlockStore::open takes the committee.
 * One image runs on one device (the context's first), as mv_wal_verify; takes the context in turn. */
mv_status mv_wal_replay(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                        uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap, uint64_t* count,
                        uint64_t* blk_rows /* cap_blocks x 10 */, uint8_t* blk_status /* cap_blocks, may be NULL */,
                        uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* summary /* 3 */,
                        uint64_t* last_seen /* committee size */);

/* Host-only helper: WalWriter::writev positions of n entries of payload_len[i] bytes written from
 * writer position `start` (an entry that would straddle a map starts at the next one); returns
 * the writer position after them. */
uint64_t mv_wal_layout(const uint64_t* payload_len, uint64_t n, uint32_t map_bits, uint64_t start,
                       uint64_t* pos /* n */);

/* The WAL write: the bytes WalWriter::writev appends for n entries (wal.rs:150-188: the crc32 of the
 * payload, the 16-byte header of combine_header, wal.rs:211-216, and the zero padding of an entry
 * that would straddle a map), as BlockWriter::insert_block and OwnBlockData::write_to_wal call it
 * for every processed block and for the own block (block_store.rs:504-518, 542-549). The inverse of
 * mv_wal_replay: a caller appends out[0 .. *end_pos - start) to its file with one pwrite in place of
 * n write_vectored calls.
 *
 * entries: n rows of 4 uint64_t words, mirroring the replay's block rows:
 *   [0] tag (its low 32 bits; opaque, the writer does not judge it)
 *   [1] offset of the payload in buf   [2] its length   [3] OwnBlockData::next_entry
 * For tag 3 (WAL_ENTRY_OWN_BLOCK) the eight little-endian bytes of word [3] are written in front of
 * the payload and are covered by the crc and by len: what writev(WAL_ENTRY_OWN_BLOCK, &[header,
 * block]) produces. For every other tag word [3] is ignored. A zero-length payload is an entry
 * (len 16, crc 0). start = the writer position before the call (WalWriter::pos, at most 2^62);
 * maps of 2^map_bits bytes, 8 <= map_bits <= 30, as mv_wal_verify.
 *
 * out[0 .. *end_pos - start): exactly the bytes write_vectored appends to a file of length `start`
 * -- per entry the zero gap if the entry would straddle a map (wal.rs:164-172; written as zero
 * whatever out held), the header combine_header(crc, len, tag).to_le_bytes() with len = body + 16
 * and crc = crc32fast::hash(body) as a u64, then the body. No byte at or past *end_pos - start is
 * touched. pos[i] = the WalPosition.start of entry i (what insert_block stores in the index; the
 * positions are mv_wal_layout's), *end_pos = the writer position after the call.
 *
 * Decided before any byte of out is written: MV_E_INVALID_ARG, with out untouched and *end_pos =
 * start, for a body longer than 2^map_bits - 16 (the assert of wal.rs:153) and for a payload that
 * leaves buf[0, buf_bytes). If *end_pos - start exceeds cap no byte of out is written, but pos and
 * *end_pos are: call again with room (the rule of mv_encode_blocks). cap may be 0 and out NULL to
 * size only; n may be 0 (*end_pos = start). buf and out do not overlap.
 * Cost: the bytes are written by one wave per entry; the positions take one scan and then one
 * dependent search per map the image touches, resolved one after another by a single wave while
 * the call holds the context -- time proportional to (*end_pos - start) / 2^map_bits on top of the
 * scan (a few steps at map_bits 24; at map_bits 8 about one per entry, which only test sizes bear).
 * Runs on the context's first device; takes the context in turn. */
mv_status mv_wal_write(mv_ctx* ctx, const uint8_t* buf, uint64_t buf_bytes, const uint64_t* entries /* n x 4 */,
                       uint64_t n, uint64_t start, uint32_t map_bits, uint8_t* out, uint64_t cap,
                       uint64_t* pos /* n */, uint64_t* end_pos);

/* Host-only helper: the Data<StatementBlock> byte strings inside received network frames
 * (Network::handle_read_stream, network.rs:400-447: a u32 big-endian size, then
 * bincode(NetworkMessage), network.rs:36-46; size 0 is a ping followed by 8 bytes). Lists the
 * blocks of every Blocks / RequestBlocksResponse message in buf[0, len) (u32 tag 1 or 3, u64
 * count, then u64 length + bytes per block, data.rs:67-96) as offsets into buf and lengths, in
 * stream order, for mv_verify_blocks on the same buffer (no copy of the bytes); the other
 * messages and pings are skipped unparsed. Stops before an incomplete trailing frame, and
 * *consumed (optional) = the bytes of the complete frames. Returns the number of blocks found
 * (the first `cap` written; cap 0 only counts), or -1 where the reference drops the connection:
 * a size above MAX_SIZE = 16 MiB (network.rs:216-221), a message tag above 4, or a block count
 * or length that runs past its frame (a bincode error, network.rs:454-457). */
int64_t mv_frame_blocks(const uint8_t* buf, uint64_t len, uint64_t* off, uint64_t* blen, uint64_t cap,
                        uint64_t* consumed);

/* Received bytes verified per message (replaces, for many connections at once: the frame reads of
 * Network::handle_read_stream, network.rs:400-447; bincode::deserialize::<NetworkMessage>,
 * network.rs:454-457, which decodes every inner block, data.rs:83-96, before any is verified;
 * and NetworkSyncer::process_blocks, net_sync.rs:314-383, which returns Err at the first
 * rejected block, before add_blocks, and so ends the connection).
 *
 * Stream s is one connection's received bytes buf[soff[s], soff[s] + slen[s]); streams are only
 * read and may overlap. A frame is a u32 big-endian size and that many bytes of
 * bincode(NetworkMessage); size 0 is a ping with 8 more bytes (no message, no row). The walk of a
 * stream stops before an incomplete trailing frame; consumed[s] = the bytes of the complete frames
 * walked. Every other frame yields one message row of 8 uint32_t words, rows flat across streams
 * in stream order, then arrival order:
 *   [0] stream   [1] message tag   [2] [3] off: offset in buf of the frame's size word (low, high)
 *   [4] first_block  [5] n_blocks: the message's blocks are blk_off / blk_len / blk_status
 *       [first_block, first_block + n_blocks)
 *   [6] status | bad_status << 8   [7] bad_block, or 0xFFFFFFFF
 * status is MV_MSG_*:
 *   OK                  the message decodes and all its blocks are MV_BLOCK_OK (messages without
 *                       blocks and Blocks of count 0, net_sync.rs:320-322, included)
 *   DECODE_ERROR        size < 4; tag > 4; tag 0 (Subscribe) with fewer than 8 body bytes; tags 1 / 3
 *                       (Blocks, RequestBlocksResponse) whose count or a block length runs past the
 *                       frame; tags 2 / 4 (RequestBlocks, BlockNotFound) with a BlockReference (u64,
 *                       u64, u64 digest length, digest; types.rs:49-54, crypto.rs:322-347) that runs
 *                       past the frame or whose digest length is not 32; or a block of a tag 1 / 3
 *                       message is MV_BLOCK_PARSE_ERROR: bad_block = the first such block. This wins
 *                       over an earlier rejected block of the message (the decode comes first).
 *   BLOCK_REJECTED      every block parses; bad_block = the first one not MV_BLOCK_OK (its index in
 *                       the message), bad_status = its MV_BLOCK_*
 *   TOO_MANY_REQUESTED  a well-formed RequestBlocks of more than 50 references (BlockNotFound has
 *                       no limit)
 *   NOT_REACHED         the message follows the first message of its stream that is not OK
 *   BAD_SIZE            size above 16 MiB
 * The tag word is 0xFFFFFFFF where no tag was read (BAD_SIZE, and a DECODE_ERROR of size < 4).
 * Trailing bytes after the message inside its frame are allowed (as mv_frame_blocks allows them).
 * drop_msg[s] = the flat index of stream s's first row that is not OK, or 0xFFFFFFFF.
 * The walk itself stops a stream at the first row the bytes alone condemn (BAD_SIZE: consumed
 * ends before that frame; a frame-level DECODE_ERROR or TOO_MANY_REQUESTED: after it); a message
 * whose count or length overruns lists no blocks (n_blocks 0). Messages after a row that turns
 * bad only through a block verdict are still walked and their blocks verified; their rows
 * then become NOT_REACHED.
 * The reference skips blocks it has processed before (net_sync.rs:331-335) ahead of verify; such
 * a block passed the same deterministic check then, so verifying it again changes no verdict
 * (mv_accept_blocks does skip them, on the index of block references).
 *
 * mv_frame_messages: host only, one stream buf[0, len), stream word 0. The rows carry the
 * statuses the bytes alone decide (OK, frame-level DECODE_ERROR, TOO_MANY_REQUESTED, BAD_SIZE) and
 * the walk stops after the first that is not OK; every listed block belongs to a row, and tags
 * 0, 2 and 4 are bound-checked. Returns the number of rows (the first cap_msgs written, and the
 * first cap_blocks blocks; *n_blocks = blocks found), or -1 for bad arguments. */
int64_t mv_frame_messages(const uint8_t* buf, uint64_t len, uint32_t* msgs /* cap_msgs x 8 */, uint64_t cap_msgs,
                          uint64_t* blk_off, uint64_t* blk_len, uint64_t cap_blocks, uint64_t* n_blocks,
                          uint64_t* consumed);
/* mv_verify_frames: ns streams of host buffer buf. On the device: the frame walk, the message
 * walk, StatementBlock::verify of every listed block in place (the block path of
 * mv_dev_verify_blocks: the comb kernels below MV_BATCH_MIN blocks per device, the walk / batch
 * path from there), the message and stream verdicts. Requires mv_set_committee; takes the
 * context in turn. Only the first cap_msgs rows and cap_blocks blocks are written; *n_msgs and
 * *n_blocks are always the totals. blk_status (MV_BLOCK_*, optional) may be NULL. Several devices
 * or logical shards: whole streams are split by bytes (mv_shard_plan weights slen + 64), and row
 * and block indices are rebased, so the result does not depend on the split. Streams in
 * page-locked memory (mv_host_alloc), in order and disjoint, are DMAd in place as
 * mv_verify_blocks does; others are packed stream by stream first. */
mv_status mv_verify_frames(mv_ctx* ctx, const uint8_t* buf, const uint64_t* soff, const uint64_t* slen, uint32_t ns,
                           uint64_t* consumed /* ns */, uint32_t* drop_msg /* ns */, uint32_t* msgs /* cap_msgs x 8 */,
                           uint64_t cap_msgs, uint64_t* n_msgs, uint64_t* blk_off, uint64_t* blk_len,
                           uint8_t* blk_status /* may be NULL */, uint64_t cap_blocks, uint64_t* n_blocks);

/* ---- the index of block references ----
 * A set of BlockReferences in device memory (the context's first device), keyed by the 48 bytes of a
 * reference as six little-endian uint64_t words -- authority, round, the four digest words: words
 * 3..8 of an mv_wal_replay row -- with a state each (MV_REF_*). It answers what the core answers
 * around verify: BlockManager::exists_or_pending is "the entry is MV_REF_HAVE" (block_manager.rs:142-144),
 * BlockManager::missing_blocks is the MV_REF_WANTED entries (:138-140). The genesis references are in
 * the reference's store from the start (block_store.rs:50-62, types.rs:141-150): the caller inserts
 * them as MV_REF_HAVE. The index is made on first use; every call takes the context in turn.
 *
 * mv_index_reserve: makes the index, or grows it so that `entries` entries fit at a load of at most
 * 1/2 (the entries are rehashed on the device). Never shrinks. mv_index_clear empties it. */
mv_status mv_index_reserve(mv_ctx* ctx, uint64_t entries);
mv_status mv_index_clear(mv_ctx* ctx);
/* out[0] HAVE entries (MV_REF_STORED ones among them), out[1] WANTED entries, out[2] the capacity in entries, out[3] rebuilds so far,
 * out[4] the longest probe (slots examined) of any insert or lookup since the last clear. */
mv_status mv_index_stats(mv_ctx* ctx, uint64_t* out /* 5 */);
/* Raises n references to `state` (MV_REF_WANTED or MV_REF_HAVE): absent ones are entered, a WANTED one
 * becomes HAVE (block_manager.rs:100: an arriving block leaves `missing`), nothing is lowered.
 * prior[i] (optional) = the state of refs[i] before the call, for every duplicate inside the call
 * too. Grows the index as needed. */
mv_status mv_index_insert(mv_ctx* ctx, const uint64_t* refs /* n x 6 */, uint64_t n, uint32_t state,
                          uint8_t* prior /* n, may be NULL */);
/* mv_index_insert towards MV_REF_STORED (which mv_index_insert itself goes on refusing): the
 * references of blocks that are in the store -- the genesis blocks, the blocks of a replayed WAL, the
 * caller's own proposed block. A caller that wants mv_connect_blocks to release anything seeds these
 * as STORED, not HAVE: a block connects only when every include is STORED. */
mv_status mv_index_insert_stored(mv_ctx* ctx, const uint64_t* refs /* n x 6 */, uint64_t n,
                                 uint8_t* prior /* n, may be NULL */);
/* state[i] = MV_REF_* of refs[i] (BlockStore::block_exists || blocks_pending.contains_key for HAVE,
 * block_manager.rs:68-69). */
mv_status mv_index_lookup(mv_ctx* ctx, const uint64_t* refs /* n x 6 */, uint64_t n, uint8_t* state /* n */);
/* The MV_REF_WANTED entries (BlockManager::missing_blocks, block_manager.rs:138-140, which the
 * synchronizer reads, synchronizer.rs:335), in no particular order: *n = how many there are, the
 * first `cap` written. */
mv_status mv_index_wanted(mv_ctx* ctx, uint64_t* refs /* cap x 6 */, uint64_t cap, uint64_t* n);
/* One accept call: process_blocks (net_sync.rs:314-386) for n received blocks buf[off[i], off[i] +
 * len[i]) of the messages grp[i] (non-decreasing; NULL: every block is a message of its own), up to
 * and including what BlockManager::add_blocks reports missing (block_manager.rs:48-136). It restates
 * one interleaving of the reference's peer tasks: every task's `processed` query ran before any
 * add_blocks.
 *  1. A block is KNOWN when its own reference (bytes 0..56, read only when len >= 56, digest length
 *     word 32) is MV_REF_HAVE in the index as it stood before the call. KNOWN blocks are not
 *     verified and cannot reject their message, whatever their body holds (net_sync.rs:333-336).
 *  2. The others go through StatementBlock::verify as in mv_dev_verify_blocks (the comb kernels below
 *     MV_BATCH_MIN blocks, the walk / batch path from there, chunks of max_batch).
 *     blk_status[i] = MV_BLOCK_*, MV_BLOCK_OK for KNOWN blocks.
 *  3. A message is accepted when all its blocks are KNOWN or OK; else its blocks that are not KNOWN
 *     are MV_ACC_DROPPED (OK) or MV_ACC_REJECTED: process_blocks returns before add_blocks (:352-361).
 *  4. Of the OK blocks of accepted messages with one reference the lowest index is MV_ACC_NEW, the
 *     others MV_ACC_DUP (block_manager.rs:68-72). The references of NEW blocks become MV_REF_HAVE.
 *  5. The includes of NEW blocks (u64 count at byte 56, 56 bytes each from byte 64) that have no
 *     entry after step 4 become MV_REF_WANTED and are listed in `missing`, each once, ordered by
 *     (block, include) of their first occurrence: the missing_references of add_blocks (:82-88).
 *     An include that is a NEW block of the same call is not missing (add_blocks sorts by round, :57;
 *     this holds across the messages of one call too: their accepted blocks count as one vector).
 * *n_missing is the total; nothing is written past min(*n_missing, cap_missing) rows. Page-locked
 * (mv_host_alloc), ordered, disjoint blocks are DMAd in place as mv_verify_blocks does; others are
 * packed. Grows the index as needed. The suspend / unlock cascade of add_blocks (blocks_pending,
 * :102-131) is mv_connect_blocks'; with this call it and the WAL write stay with the caller.
 * Requires mv_set_committee. */
mv_status mv_accept_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                           const uint64_t* grp /* n, may be NULL */, uint32_t n, uint8_t* blk_status /* n */,
                           uint8_t* blk_state /* n */, uint64_t* missing /* cap_missing x 6 */, uint64_t cap_missing,
                           uint64_t* n_missing);
/* mv_accept_blocks and the suspend / unlock cascade of add_blocks (block_manager.rs:102-131): the
 * whole of BlockManager::add_blocks but the block bodies and the WAL write. Steps 1-5 are those of
 * mv_accept_blocks. Then:
 *  6. Every NEW block joins the context's suspended-block store (device memory: its own reference,
 *     its includes, its arrival position) in block order, and the store is swept level by level:
 *     S_0 is the set of MV_REF_STORED references after step 5; level l connects every suspended
 *     block that is not in S_l and whose includes are all in S_l (a block without includes
 *     connects); their references rise to MV_REF_STORED, and S_l+1 is S_l with them. The sweep ends
 *     at the first level that connects nothing. Connected blocks leave the store; what stays is
 *     blocks_pending. (An include of a suspended block is a key of block_references_waiting exactly
 *     while it is not stored, so this is the unlock test of :120-123, and the result is add_blocks'
 *     newly_blocks_processed as a set.)
 * connected row k is 8 words: 0-5 the reference, 6 the block's index in this call (UINT64_MAX: an
 * earlier call suspended it), 7 its level. Rows are ordered by level and, within a level, by
 * arrival: blocks suspended by earlier calls first, in the order they were suspended, then this
 * call's by index. The order is causal: every include of a row was STORED before the call or stands
 * in an earlier row. *n_connected is the total; nothing is written past min(*n_connected,
 * cap_connected) rows, and the states rise in full whatever the cap.
 * blk_state: a NEW block that connected stays MV_ACC_NEW, one that was parked is MV_ACC_SUSPENDED.
 * n = 0 is a sweep alone, for after the caller raised references with mv_index_insert_stored.
 * A context whose genesis references were seeded as MV_REF_HAVE never connects anything.
 * Grows the index and the store as needed. Results do not depend on MV_INDEX_TAG_BITS.
 * After an error from this call (or its device-buffer variant) other than MV_E_INDEX_FULL and
 * MV_E_INVALID_ARG, which leave index and store as they were, references of the call's blocks may
 * be MV_REF_HAVE without a record in the store: such blocks would be KNOWN from then on and never
 * connect. The caller then empties both with mv_index_clear and seeds again. */
mv_status mv_connect_blocks(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len,
                            const uint64_t* grp /* n, may be NULL */, uint32_t n, uint8_t* blk_status /* n */,
                            uint8_t* blk_state /* n */, uint64_t* missing /* cap_missing x 6 */, uint64_t cap_missing,
                            uint64_t* n_missing, uint64_t* connected /* cap_connected x 8 */, uint64_t cap_connected,
                            uint64_t* n_connected);
/* Room in the suspended-block store for `blocks` blocks with `includes` includes in all (never
 * shrinks); mv_index_clear empties the store, mv_destroy frees it. */
mv_status mv_pending_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t includes);
/* out[0] MV_REF_STORED entries, out[1] suspended blocks, out[2] their includes, out[3] the levels
 * (that connected something) of the last connect call. */
mv_status mv_pending_stats(mv_ctx* ctx, uint64_t* out /* 4 */);

/* ---- the DAG store and the direct decision rule ----
 * Opt-in: after mv_dag_reserve, mv_connect_blocks (and its device-buffer variant) copies every block
 * it connects -- the slot of its reference, its (authority, round), its includes as slots of the
 * index -- into the context's DAG store before the suspended-block store drops it. Records stand in
 * the order blocks became MV_REF_STORED: the connected-row order, call after call. Without the
 * reserve, mv_connect_blocks does what it did before, launch for launch. The store grows
 * geometrically, also under the device-buffer connect call (which synchronises anyway);
 * mv_index_clear empties it, mv_destroy frees it, a rebuild of the index re-resolves its slots.
 * References seeded with mv_index_insert_stored / mv_dev_index_insert (genesis, a replay's rows
 * seeded that way) have no record; a replay's rows get theirs from mv_wal_recover /
 * mv_dev_dag_seed_rows. A missing record is safe because the rule below is monotone in the records
 * (see mv_decide_leaders). */
mv_status mv_dag_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t includes);
/* Drops the records of rounds below `round` by stable compaction: BlockStore::cleanup /
 * unload_below_round (block_store.rs:207-218, 374-390) for this store. The index entries stay
 * (a state never falls); an include whose record was pruned reads "no record", like one that
 * never had any. MV_E_INVALID_ARG without a store. */
mv_status mv_dag_prune(mv_ctx* ctx, uint64_t round);
/* out[0] records, out[1] their includes, out[2] the lowest and out[3] the highest round of a record
 * (both 0 without records). All 0 without a store. */
mv_status mv_dag_stats(mv_ctx* ctx, uint64_t* out /* 4 */);

#define MV_LEADER_UNDECIDED 0 /* LeaderStatus::Undecided: neither rule holds on the records there are */
#define MV_LEADER_COMMIT 1    /* LeaderStatus::Commit(block): words 0-5 are the block's reference */
#define MV_LEADER_SKIP 2      /* LeaderStatus::Skip: a quorum of blame (base_committer.rs:326-329) */
#define MV_LEADER_CONFLICT 3  /* more than one leader block with enough support: the reference panics (:347-352) */
#define MV_LEADER_OVERFLOW 4  /* more than MV_DECIDE_MAX_LEADER_BLOCKS leader blocks: not a verdict, the caller
                                 decides this leader itself */
#define MV_DECIDE_MAX_LEADER_BLOCKS 8
/* BaseCommitter::try_direct_decide (base_committer.rs:323-357) at wave length 3 (core.rs:127-129 never
 * calls with_wave_length; DEFAULT_WAVE_LENGTH = MINIMUM_WAVE_LENGTH = 3), for each of n leader rows
 * (authority a, round r) on its own. The caller elects the leaders (Committee::elect_leader,
 * committee.rs:137-147, is host logic). The stored blocks are the DAG store's records; a quorum is
 * stake > quorum_threshold (committee.rs:125-127). A verified block's includes all have a lower
 * round than the block (threshold_clock.rs:18-22), so find_support (:109-134) never recurses here.
 *   Voting blocks: the records of round r + 1. Decision blocks: those of round r + 2. Leader
 *   blocks: those with (authority, round) = (a, r).
 *   Blame (enough_leader_blame, :228-249): the authors of voting blocks none of whose includes has
 *   authority a -- the authority only, never the round (:234-237). A quorum of them: MV_LEADER_SKIP.
 *   The support of a voting block V: the first include of V, in include order, with (authority,
 *   round) = (a, r), or none. V votes for leader block B when that include is B's reference (is_vote, :138-145).
 *   A decision block C is a certificate for B (is_certificate, :152-180) when the authors of those
 *   includes of C that have a record, are of round r + 1 and vote for B are a quorum; an author
 *   counts once, however many of its blocks C includes.
 *   B has enough support (enough_leader_support, :253-289) when the authors of its certificates are
 *   a quorum. (The total_stake quick reject of :261-273 cannot change a result and is left out.)
 *   Exactly one leader block with enough support: MV_LEADER_COMMIT. More than one:
 *   MV_LEADER_CONFLICT. None: MV_LEADER_UNDECIDED. The blame test comes first, as in the reference.
 *   More than MV_DECIDE_MAX_LEADER_BLOCKS leader blocks, and no quorum of blame: MV_LEADER_OVERFLOW.
 * out row i: words 0-5 the committed block's reference (else a, r and four zero words), 6 the
 * status, 7 the leader blocks found. stakes row i (stakes may be NULL): the blame stake; the vote
 * stake -- the distinct authors of voting blocks that vote for the block -- of the one block with
 * enough support, else of the leader block with the largest (vote stake, certificate stake) pair;
 * the certificate stake of that same block. They are whole sums without early exit. Both are 0
 * under more than MV_DECIDE_MAX_LEADER_BLOCKS leader blocks.
 * A row whose authority is not in the committee is MV_LEADER_UNDECIDED with 0 leader blocks and 0
 * stakes. A leader whose round lies below the store's lowest record round (or any, in an empty
 * store) is MV_LEADER_UNDECIDED.
 * Monotone: a block without a record can only lower a stake. So a store that lacks edges (seeded
 * references, pruned rounds, blocks still suspended) turns COMMIT or SKIP into UNDECIDED, never the
 * reverse, and never one COMMIT into another. (Where authors of more than a third of the stake
 * equivocate in the voting round, a quorum of blame can stand beside a leader block with enough
 * support; blame is tested first, here as in the reference, so fewer records can uncover that COMMIT.)
 * What stays with the caller: try_indirect_decide (:294-318), the longest-decided-prefix rule and
 * the genesis filter of UniversalCommitter::try_commit (mv_commit_leaders runs these); the linearizer is
 * mv_linearize.
 * Requires mv_set_committee (MV_E_NO_COMMITTEE) and mv_dag_reserve (MV_E_INVALID_ARG without the
 * store). n = 0 does nothing. Results do not depend on MV_INDEX_TAG_BITS, on the order blocks were
 * delivered in, or on launch geometry. */
mv_status mv_decide_leaders(mv_ctx* ctx, const uint64_t* leaders /* n x 2: authority, round */, uint32_t n,
                            uint64_t* out /* n x 8 */, uint64_t* stakes /* n x 3, may be NULL */);

#define MV_COMMIT_KIND_NONE 0     /* info word 0: the row is not decided */
#define MV_COMMIT_KIND_DIRECT 1   /* the direct rule gave the row's status */
#define MV_COMMIT_KIND_INDIRECT 2 /* the indirect rule did, from the anchor of word 1 */
#define MV_COMMIT_INCOMPLETE 1    /* info word 2, bit 0: the store lacks records this row's walk would read */
#define MV_COMMIT_BLOCKED 2       /* bit 1: the first row three rounds up that is not SKIP is not COMMIT either */
/* What UniversalCommitter::try_commit returns (consensus/universal_committer.rs:30-90), at wave length
 * 3: the direct rule of mv_decide_leaders, BaseCommitter::try_indirect_decide (base_committer.rs:294-318)
 * for the rows it leaves undecided, and the longest decided prefix. `leaders` holds the rows in the
 * order try_commit's deque ends in (:38-72: rounds downwards, committers in reverse, push_front):
 * ascending round, and within a round in committer order. The caller elects them and starts after its
 * last_decided leader (:46-53). Rows not in non-decreasing round order: MV_E_INVALID_ARG.
 * For row i = (a, r), from the last row to the first:
 *   Direct first. The row's status under mv_decide_leaders; anything but MV_LEADER_UNDECIDED is
 *   final, kind MV_COMMIT_KIND_DIRECT.
 *   Anchor scan (:299-315). Otherwise the rows j > i with round_j >= r + 3, in row order: a SKIP row is
 *   passed over, a COMMIT row is the anchor, any other row stops the scan and row i stays
 *   MV_LEADER_UNDECIDED with MV_COMMIT_BLOCKED. Without an anchor the row stays MV_LEADER_UNDECIDED.
 *   Reach (BlockStore::linked_to_round, block_store.rs:306-327). With the anchor's block A at round R,
 *   reach[R] = {A}; for q = R - 1 down to r + 2, reach[q] = the records of round q that are an include
 *   of a record in reach[q + 1]. Only includes exactly one round below the including block carry the
 *   walk, as in the reference's loop; an empty level ends it (:322-324).
 *   Certificates (decide_leader_from_anchor, base_committer.rs:184-224). The leader blocks are the
 *   records with (authority, round) = (a, r); more than MV_DECIDE_MAX_LEADER_BLOCKS: MV_LEADER_OVERFLOW.
 *   Leader block B is certified when some C in reach[r + 2] is a certificate for B, by the predicate of
 *   mv_decide_leaders. Exactly one certified block: MV_LEADER_COMMIT of it. More than one:
 *   MV_LEADER_CONFLICT (the reference panics, :214-216). None: MV_LEADER_SKIP -- unless the row is
 *   incomplete. These are kind MV_COMMIT_KIND_INDIRECT.
 *   Incomplete. The direct rule is monotone in the records; the indirect SKIP is not, since a
 *   missing record can hide the certificate. The reference never lacks a block of a stored block's
 *   sub-DAG ("We should have the whole sub-dag by now", :128, :166); this store does, for seeded
 *   references and pruned rounds. A row is incomplete when r lies below the store's lowest record
 *   round; or a record in reach[q + 1] has an include whose round is q and which has no record, for a
 *   q of the row's walk; or a record in reach[r + 2] has an include of round r + 1 without a record; or
 *   such an include has a record whose support for (a, r) is a reference without a record. An
 *   incomplete row without a certified block is MV_LEADER_UNDECIDED (kind MV_COMMIT_KIND_NONE),
 *   never SKIP; with exactly one it is still COMMIT, because missing records only remove certificates.
 *   Every row that had an anchor reports MV_COMMIT_INCOMPLETE as it was found.
 * The sequence (:75-90): the rows of round 0 are dropped first; *n_sequence is then the number of rows
 * in the longest prefix whose status is MV_LEADER_COMMIT or MV_LEADER_SKIP -- the rows of round > 0,
 * in order, up to that count.
 * out row i: as mv_decide_leaders (words 0-5 the committed reference, 6 the status, 7 the leader
 * blocks found). info row i: word 0 the kind, 1 the anchor's row (all ones without one), 2 the flags,
 * 3 the records in reach[r + 2].
 * What stays with the caller: leader election and last_decided (the linearizer is mv_linearize).
 * Requirements and refusals as mv_decide_leaders; n = 0 sets *n_sequence = 0. The call leaves no
 * state behind: a later mv_decide_leaders or mv_commit_leaders reads the store alone. */
mv_status mv_commit_leaders(mv_ctx* ctx, const uint64_t* leaders /* n x 2, in sequence order */, uint32_t n,
                            uint64_t* out /* n x 8 */, uint64_t* info /* n x 4 */, uint64_t* n_sequence);

#define MV_LINEAR_OK 0
#define MV_LINEAR_INCOMPLETE 1 /* the leader, or a block of its sub-DAG above round 0, has no record */
#define MV_LINEAR_COMMITTED 2  /* the leader is already marked (the reference asserts) */
#define MV_LINEAR_OVERFLOW 3   /* a path deeper than MV_LINEAR_MAX_DEPTH, an include number above
                                  MV_LINEAR_MAX_INCLUDE, or the sub-DAG does not fit in cap */
#define MV_LINEAR_STOPPED 4    /* a row behind the first row that is not OK */
#define MV_LINEAR_MAX_DEPTH 16
#define MV_LINEAR_MAX_INCLUDE 65534
#define MV_LINEAR_MAX_LEADERS 65535
/* Linearizer::handle_commit (consensus/linearizer.rs:125-166): every committed leader block becomes
 * its CommittedSubDag, the blocks in the reference's own order. State per context, beside the DAG
 * store: a committed mark per reference (Linearizer::committed) and last_height.
 * The reference marks a block when it is pushed and expands it when it is popped, so a block belongs
 * to the includer that is popped first, and an includer's round is higher than the block's. The pop
 * order is therefore the preorder of a tree that is built round by round, top down. For leader block
 * L of round R that is not marked:
 *   1. path(L) = (), L is marked, the sub-DAG is {L}.
 *   2. For q = R - 1 down to 0: every unmarked reference b whose key round is q and that is include
 *      number j (from 0 in include order, duplicates counted) of a member x. Of all such (x, j) the
 *      least pair (path(x), j) -- paths compare component by component, a prefix before its
 *      extensions -- gives path(b) = path(x) ++ (0xffff - j); b is marked and joins.
 *   3. The members sorted by (round, path), both ascending: collect_sub_dag and the stable
 *      sort_by_key(round). last_height += 1.
 * Leaders are taken in the order given; each sees the marks of those before it.
 * Where this store differs from the reference's (which has every block of a stored block's sub-DAG):
 * an unmarked include without a record whose round is 0 (seeded genesis) is a leaf, put out and
 * marked; one whose round is above 0 makes the leader MV_LINEAR_INCOMPLETE, as a leader without a
 * record is; a marked reference is passed over with or without a record.
 * A path holds MV_LINEAR_MAX_DEPTH components: a member whose least pair has an x that deep, or a
 * j above MV_LINEAR_MAX_INCLUDE, makes the leader MV_LINEAR_OVERFLOW and does not join. A leader that
 * meets more than one of these reports the highest status number.
 * blocks: the sub-DAGs one behind the other, six words per block; *n_rows the rows written.
 * sub row i: word 0 the status, 1 the first row, 2 the count, 3 the height. A leader whose rows do
 * not fit in cap is MV_LINEAR_OVERFLOW. Rows behind the first row that is not OK are MV_LINEAR_STOPPED;
 * a row that is not OK has first row = *n_rows, count 0, height 0.
 * State changes only for the OK prefix: a row that is not OK leaves marks and height as its OK
 * predecessors left them. The caller then linearizes that leader itself and reports it with
 * mv_linearize_mark.
 * Requires mv_dag_reserve (MV_E_INVALID_ARG without it); more than MV_LINEAR_MAX_LEADERS leaders:
 * MV_E_INVALID_ARG. n = 0 does nothing. mv_index_clear empties marks and height; index rebuilds,
 * store growth and mv_dag_prune keep them (marks are held per slot of the index). */
mv_status mv_linearize(mv_ctx* ctx, const uint64_t* leaders /* n x 6 references, sequence order */, uint32_t n,
                       uint64_t* blocks /* cap x 6 */, uint64_t cap, uint64_t* sub /* n x 4 */, uint64_t* n_rows);
/* Linearizer::recover_state (linearizer.rs:108-121), and the report after a row that was not OK:
 * marks the references and sets last_height = max(last_height, height). Every reference goes
 * through mv_index_insert_stored's insert: one without an index entry gets one, and an entry that
 * is MV_REF_WANTED or MV_REF_HAVE rises to MV_REF_STORED -- a committed block is a stored block
 * (the reference commits only what its block store holds), so a later connect call counts it as
 * an include that is there, and mv_index_wanted no longer lists it. */
mv_status mv_linearize_mark(mv_ctx* ctx, const uint64_t* refs /* n x 6 */, uint64_t n, uint64_t height);
/* out[0] = the marked references, out[1] = last_height */
mv_status mv_linearize_stats(mv_ctx* ctx, uint64_t* out /* 2 */);

/* ---- proposing: the threshold clock, the pending queue, the include choice ----
 * What stands between mv_connect_blocks and mv_seal_blocks in Core (core.rs): the
 * ThresholdClockAggregator (threshold_clock.rs:37-94), the `pending` queue and the include choice of
 * Core::try_new_block. Opt-in state on the context's first device, beside the DAG store: the clock
 * (round, voters, stake), the queue (per entry: include or payload, an include's reference as a slot
 * of the index and its round, the caller's tag), the own last block (its reference and its includes,
 * as slots), the choice of a take that mv_propose_own has not confirmed yet, and a stamp per slot of
 * the index. Without mv_propose_reserve every other call does what it did before, launch for launch,
 * and every call below is MV_E_INVALID_ARG. mv_index_clear empties the state (clock at round 0, empty
 * queue, no own block), mv_destroy frees it, a rebuild of the index re-resolves its slots. */
#define MV_PROPOSE_IN_ORDER 1   /* mv_propose_add: take the rows in the order given */
#define MV_PROPOSE_PAYLOAD 2    /* mv_propose_add: one payload entry behind the rows */
#define MV_PROPOSE_INCOMPLETE 1 /* mv_propose_take, out[3]: a taken include of round > 0 has no record */
#define MV_PROPOSE_SHORT 2      /* mv_propose_take, out[3]: cap or cap_p was too small; nothing was taken */
/* Opt in for `authority` (a seat of the committee, MV_E_NO_COMMITTEE without one), with room for
 * `entries` queue entries (never shrinks; the queue grows as needed): the clock of
 * ThresholdClockAggregator::new(0) (core.rs:88), an empty queue, no own block. */
mv_status mv_propose_reserve(mv_ctx* ctx, uint32_t authority, uint64_t entries);
/* The loop of Core::add_blocks over the processed blocks (core.rs:181-200) and the entry of
 * run_block_handler (core.rs:223-224). rows: n references, words 0-5 of each stride_words words -- the
 * connected rows of mv_connect_blocks as they are at a stride of 8. They are sorted by round, stably
 * (core.rs:181-183); each goes through ThresholdClockAggregator::add_block (threshold_clock.rs:58-89)
 * and joins the queue as an include entry with its tag (the block's WAL position; 0 without tags).
 *   Less (:61): nothing. Greater (:63-67): the set is cleared, the author added, the round set -- the
 *   quorum answer of that add is ignored. Equal (:68-87): the author is added, once per round, and
 *   when StakeAggregator::add answers true (committee.rs:314-320: stake > quorum_threshold, also for an
 *   author counted before) the set is cleared and the round is the block's + 1.
 * MV_PROPOSE_IN_ORDER skips the sort: the replay of the recovered `pending` in Core::open
 * (core.rs:90-94) and its genesis loop (:104-109). With MV_PROPOSE_PAYLOAD one payload entry carrying
 * payload_token follows the rows (n = 0: that entry alone).
 * Every row must have an entry in the index and an authority of the committee: otherwise
 * MV_E_INVALID_ARG, and clock and queue are as they were.
 * out: 0 the clock round after the call, 1 the aggregator's stake, 2 its voters, 3 the queue's length. */
mv_status mv_propose_add(mv_ctx* ctx, const uint64_t* rows, uint64_t n, uint64_t stride_words /* >= 6 */,
                         const uint64_t* tags /* n, may be NULL */, uint32_t flags, uint64_t payload_token,
                         uint64_t* out /* 4 */);
/* The include choice of Core::try_new_block (core.rs:232-278). Clock round <= the own last block's
 * round (:233-235): out[0] = 0, nothing changes. Otherwise
 *   1. the cut (:240-247) is the first include entry whose round is >= the clock round, else the
 *      queue's end; the entries before it are taken (:249-251);
 *   2. references_in_block (:254-263) is the includes of the own last block and of every taken include
 *      entry's block. The blocks are the DAG store's records; a taken entry without one (a seeded
 *      genesis reference, a pruned round, a replay row seeded as a reference only) adds nothing, as
 *      get_block's None does, and unless its round is 0 sets MV_PROPOSE_INCOMPLETE in out[3];
 *   3. includes (:265-271): the taken include entries that are not in that set, as references, in queue
 *      order, a reference that was queued twice twice. The own last block is not among them: the
 *      caller puts it first (:264);
 *   4. payloads (:272-276): the tokens of the taken payload entries, in queue order;
 *   5. the entries from the cut on are the queue.
 * The take is then outstanding until mv_propose_own confirms it; a take while one is outstanding, or
 * before the first mv_propose_own: MV_E_INVALID_ARG, nothing changes.
 * *n_includes and *n_payloads are the totals. If one is above its cap nothing is written past the
 * cap, out[3] has MV_PROPOSE_SHORT, out[0] = 0, and queue and state are as they were: call again with room.
 * out: 0 proposed (0 / 1), 1 the clock round (the new block's round), 2 the entries taken, 3 the flags,
 * 4 the tag of the first entry left (UINT64_MAX: none; next_entry, :311-315), 5 the queue's length.
 * Words 2 to 4 describe the cut, so they are what a take that runs computes: after a refusal for room
 * (MV_PROPOSE_SHORT) they are what the take would have taken and left, and the queue is whole; when the
 * clock round is <= the own last block's round no cut is made, and they are 0, 0 and UINT64_MAX
 * whatever the queue holds. */
mv_status mv_propose_take(mv_ctx* ctx, uint64_t* includes /* cap x 6 */, uint64_t cap, uint64_t* n_includes,
                          uint64_t* payloads /* cap_p */, uint64_t cap_p, uint64_t* n_payloads, uint64_t* out /* 6 */);
/* The own block after it was sealed (core.rs:307-320), and the own genesis block (:110-116). `ref` is
 * inserted as MV_REF_STORED, goes through add_block on the clock (:307-308, :110), and becomes the own
 * last block with its includes (:316-319); the outstanding take is dropped. With the DAG store
 * reserved its record -- slot, authority, round, the includes as slots -- joins the store (unless the
 * reference has one), so mv_decide_leaders, mv_commit_leaders and mv_linearize see the block; the
 * n = 0 sweep of mv_connect_blocks for the blocks that waited for it stays the caller's.
 * includes == NULL: the own last block followed by the outstanding take's choice, which is what the
 * caller sealed; ref's round must be that take's clock round. An explicit list (k x 6, each in the
 * index) is for genesis (k = 0, any non-NULL pointer) and for a restart. ref's authority must be the
 * reserved one. MV_E_INVALID_ARG otherwise, and nothing changes.
 * out: as mv_propose_add. */
mv_status mv_propose_own(mv_ctx* ctx, const uint64_t* ref /* 6 */, const uint64_t* includes /* k x 6 or NULL */,
                         uint64_t k, uint64_t* out /* 4 */);
/* out: 0 the clock round, 1 the aggregator's stake, 2 its voters, 3 the queue's length, 4 the own last
 * block's round, 5 a take is outstanding (0 / 1), 6 the takes so far, 7 the include entries the last
 * take dropped (core.rs:268). */
mv_status mv_propose_stats(mv_ctx* ctx, uint64_t* out /* 8 */);

/* ---- seeding the DAG store from a replayed WAL ----
 * mv_wal_replay, then one seed call over all its rows while the image is still in device memory:
 * the blocks of a WAL become stored blocks with records, which is what makes a replayed block
 * visible to BaseCommitter (replaces: BlockStore::open with add_unloaded, block_store.rs:50-116,
 * 398-404, and the recovered store Core::open hands to the committer, core.rs:97-113). Without it a
 * restarted context's store is empty and every leader whose rounds touch a replayed block stays
 * MV_LEADER_UNDECIDED with MV_COMMIT_INCOMPLETE.
 * Every output of mv_wal_replay is written as mv_wal_replay writes it. Then, over all *n_blocks rows
 * (whatever cap_blocks is) and their verdicts (computed whether or not blk_status is NULL), in row
 * order:
 *  1. References. The reference of every row (words 3..8) rises to MV_REF_STORED, whatever the row's
 *     verdict: the reference stores every block of its WAL without verifying it. seeded[0] = the rows.
 *  2. Records. A row gets a record in the DAG store when all of these hold: its verdict is
 *     MV_BLOCK_OK (both decision rules rest on "a verified block's includes all have a lower round";
 *     a genesis row is MV_BLOCK_GENESIS and gets none); its round is >= floor_round (the store holds
 *     what mv_dag_prune(floor_round) would have left; 0 keeps everything); it is the first row of the
 *     call, in row order, with its reference, and that reference has no record before the call; and
 *     its bincode fits the image: length >= 64, offset + length <= size, and 64 + 56 k <= length for
 *     the include count k at byte 56. Only a caller's mismatched arrays can break the last for an OK
 *     row: such a row gets no record, is counted in seeded[4], and its bytes are never an address.
 *     Records are appended behind those there, in row order -- WAL order is the order in which blocks
 *     became stored in the life before, as connected-row order is in this one -- with the fields a
 *     connect call writes. seeded[1] = the records appended, seeded[2] = their includes.
 *  3. Includes. The includes of a record row (56 bytes each from byte 64 of its block, at any byte
 *     alignment) are resolved to their entries. An include that is a row of the same call resolves to
 *     that row's entry wherever the row stands. An include with no entry after step 1 is entered as
 *     MV_REF_WANTED, each once, as step 5 of mv_accept_blocks enters includes, so mv_index_wanted
 *     lists it; seeded[3] counts them. A WAL the reference wrote yields 0: anything else tells the
 *     caller that its WAL is not self-contained, and the rows near the gap read MV_COMMIT_INCOMPLETE.
 * A block suspended earlier that waits for a reference this call raised is released by the next
 * mv_connect_blocks sweep (n = 0), as after mv_index_insert_stored. mv_dag_prune, rebuilds of the
 * index and later connect calls treat seeded records like any others.
 * Grows the index and the DAG store as needed. Requires mv_set_committee (MV_E_NO_COMMITTEE) and
 * mv_dag_reserve (MV_E_INVALID_ARG without the store; nothing is replayed then). A WAL without block
 * rows seeds nothing. After MV_E_HIP or MV_E_ALLOC from the seeding the caller empties index and
 * store with mv_index_clear and seeds again, as after a failed connect call. */
mv_status mv_wal_recover(mv_ctx* ctx, const uint8_t* wal, uint64_t size, uint64_t end_pos, uint32_t map_bits,
                         uint64_t* pos, uint32_t* tag, uint32_t* len, uint8_t* status, uint64_t cap, uint64_t* count,
                         uint64_t* blk_rows /* cap_blocks x 10 */, uint8_t* blk_status /* cap_blocks, may be NULL */,
                         uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* summary /* 3 */,
                         uint64_t* last_seen /* committee size */, uint64_t floor_round, uint64_t* seeded /* 5 */);

/* ---- sealing blocks ----
 * The inverse of mv_verify_blocks: StatementBlock::new_with_signer (types.rs:155-218), i.e.
 * Signer::sign_block (crypto.rs:199-223) and BlockDigest::new (crypto.rs:38-61), for n blocks that
 * are Data<StatementBlock> bincode already (types.rs:93-114, data.rs:43-52) but for their digest
 * and signature fields, which are placeholders: read by nobody, overwritten. */
#define MV_SEAL_OK 0             /* sealed */
#define MV_SEAL_PARSE_ERROR 1    /* fails what MV_BLOCK_PARSE_ERROR fails; bytes untouched */
#define MV_SEAL_UNKNOWN_AUTHOR 2 /* parses, authority >= n_auth; bytes untouched */
#define MV_SEAL_UNLINKED 3       /* MV_SEAL_LINK: an include names a block of this call of the same or a
                                    later round; bytes untouched */
#define MV_SEAL_LINK 1u          /* flags: the blocks are a DAG, see below */
/* For every block buf[off[i], off[i] + len[i]) that deserializes and whose authority < n_auth:
 *   m   = Blake2b-256 of the signed pre-image (BlockDigest::digest_without_signature,
 *         crypto.rs:85-128: what mv_block_preimage returns; neither the block's own digest nor its
 *         signature is part of it)
 *   sig = the RFC 8032 signature of m under seeds[authority] (Signer::sign_block, crypto.rs:199-223;
 *         what mv_ed25519_sign gives for that seed and m)
 *   d   = Blake2b-256(pre-image || sig) (BlockDigest::new, crypto.rs:38-61)
 * sig goes to the 64 signature bytes the bincode ends on and d to bytes 24..56 of the block (the
 * digest of its own BlockReference, the layout block_codec.h names). No other byte of buf changes,
 * between and after blocks included. Blocks must not overlap. status[i] = MV_SEAL_*; msg_digest[i]
 * = m and block_digest[i] = d (either array may be NULL), zero for a block that was not sealed.
 * A round-0 block is sealed like any other: the reference's genesis blocks carry a zero signature
 * (types.rs:141-150) and stay with the caller.
 *
 * flags & MV_SEAL_LINK seals a DAG in one call. The blocks that parse (known authority or not) must
 * stand in non-decreasing round order, else MV_E_INVALID_ARG with nothing written. The call keeps a
 * table (authority, round) -> block over its blocks that are neither parse errors nor of an unknown
 * author; of several blocks with one key the lowest index holds it. Before block i is hashed,
 * every include whose (authority, round) is a key of the table
 *   - of a round below block i's: gets the digest the call computed for that block written over
 *     its 32 digest bytes -- unless that block was itself left MV_SEAL_UNLINKED, which has no
 *     fresh digest: the include then keeps its bytes;
 *   - of block i's round or a later one: is not linked. Block i is MV_SEAL_UNLINKED and no byte
 *     of it changes (StatementBlock::verify would reject it as MV_BLOCK_INCLUDE_ROUND anyway).
 * Includes that match no key keep their bytes: genesis, and blocks sealed earlier. One device
 * step runs per distinct round, lowest first; the host reads the blocks' (authority, round) back
 * once per call, and from them checks the order, fills the table (an open-addressed hash whose
 * longest probe bounds every device lookup) and cuts the steps. Without the flag there is neither
 * table nor order: every block is sealed on its own, in one step.
 * n_auth <= 2^20; seeds may be NULL when n_auth is 0 (every block is then MV_SEAL_UNKNOWN_AUTHOR).
 * No committee is needed. Runs on the context's first device; takes the context in turn.
 * The seeds are secrets: the library's device copies of them and of the expanded keys (scalar and
 * prefix) are zeroed before the call returns; the host-buffer call reads `seeds` from the
 * caller's memory as it is (pageable or pinned), like mv_ed25519_sign. */
mv_status mv_seal_blocks(mv_ctx* ctx, uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                         const uint8_t* seeds /* n_auth x 32 */, uint32_t n_auth, uint32_t flags,
                         uint8_t* status /* n, MV_SEAL_* */, uint8_t* msg_digest /* n x 32 or NULL */,
                         uint8_t* block_digest /* n x 32 or NULL */);

/* ---- encoding blocks ----
 * What stands between mv_propose_take and mv_seal_blocks: the block of Core::try_new_block written
 * as bytes. Replaces the include and statement vectors of core.rs:264-291 (the own last block first,
 * then the take's choice; statements.extend(payload) per taken payload), the struct of
 * StatementBlock::new_with_signer (types.rs:93-114, 155-218) and Data::new's bincode::serialize
 * (data.rs:43-52). The digest and signature fields come out as the zero placeholders mv_seal_blocks
 * overwrites; MV_ENCODE_SEAL seals in the same call. Stateless: no index, store or clock changes, no
 * committee is needed. Runs on the context's first device and takes the context in turn.
 *
 * Inputs, for n blocks:
 *   heads        n x 10 words: 0 authority, 1 round, 2 / 3 the low / high half of
 *                meta_creation_time_ns, 4 epoch, 5 epoch marker (0 / 1), 6 the first row of `includes`,
 *                7 the include count k, 8 the first entry of the payload list, 9 the payload count
 *   includes     m x 6 words: the reference rows mv_propose_take writes and mv_propose_own reads. The
 *                caller puts the own last block's reference in row 0 of a block's run and the take's
 *                output behind it (core.rs:264-271)
 *   payload_buf, payload_off[p], payload_len[p]: payload j is payload_buf[payload_off[j],
 *                payload_off[j] + payload_len[j]), one bincode::serialize(&Vec<BaseStatement>) string
 *                as run_block_handler writes it into a tag-2 WAL entry (core.rs:217-224): a u64 count,
 *                then the statements; at any byte offset. A block's statements are the bodies of its
 *                payloads in list order under one count, the sum of theirs. Payloads may be shared
 *                between blocks and may overlap.
 * An OK block's bytes: authority, round, 32, 32 zero bytes; k; k x (authority, round, 32, digest); the
 * statement count; the payload bodies; time low, time high; the marker byte; the epoch; 64, 64 zero
 * bytes -- 169 + 56 k + sum(payload_len - 8) bytes. Blocks lie one behind the other in `out`, each
 * starting on an 8-byte boundary; the 0-7 bytes between a block's end and the next start are
 * written as zero. out_off[i] is where block i starts, out_len[i] its length, *out_bytes the whole
 * span (the padding of the last block included). A block that is not MV_ENCODE_OK has out_len 0, takes
 * no space (its out_off is where the next block starts) and changes nothing for its neighbours. */
#define MV_ENCODE_OK 0
#define MV_ENCODE_BAD_HEAD 1    /* marker > 1, or the include run leaves [0, m), or the payload run leaves [0, p) */
#define MV_ENCODE_BAD_PAYLOAD 2 /* a payload of the block leaves payload_buf, fails the statement walk
                                   (types.rs:100-114, what MV_BLOCK_PARSE_ERROR fails), or the walk does not end on
                                   its last byte: trailing bytes would end up between two payloads' statements */
#define MV_ENCODE_TOO_LONG 3    /* longer than MV_ENCODE_MAX_LEN: the panic of core.rs:300-306 */
/* wal.rs:107 at the production map size (wal.rs:96-97, 110): MAX_ENTRY_SIZE / 2 =
 * (0x1000000 - 16) / 2 */
#define MV_ENCODE_MAX_LEN 8388600
#define MV_ENCODE_SEAL 1u /* flags: seal the encoded blocks in place (mv_seal_blocks' body) */
#define MV_ENCODE_LINK 2u /* flags, with MV_ENCODE_SEAL: MV_SEAL_LINK */
/* status[i] = MV_ENCODE_*, checked in the order above. If *out_bytes exceeds cap the call writes no
 * byte of `out` and does not seal, but status, out_off, out_len and *out_bytes are written: call again
 * with room (the rule of MV_PROPOSE_SHORT); with MV_ENCODE_SEAL every seal_status is then
 * MV_SEAL_PARSE_ERROR and the digests are zero.
 * MV_ENCODE_SEAL: seeds, n_auth, seal_status, msg_digest and block_digest are mv_seal_blocks' (the
 * digest arrays may be NULL), run over the encoded image before anything is copied back. A block that is
 * not MV_ENCODE_OK is an empty span to the seal: its seal_status is MV_SEAL_PARSE_ERROR, its digests
 * are zero, and under MV_ENCODE_LINK the includes that name it keep their bytes. Everything else the
 * seal's comment says holds: MV_SEAL_UNLINKED, MV_SEAL_UNKNOWN_AUTHOR, rounds out of order under LINK
 * are MV_E_INVALID_ARG (then `out` is not written; status, out_off, out_len and *out_bytes are), the
 * seeds and keys are zeroed on the device. Without MV_ENCODE_SEAL the five arguments are ignored.
 * n, m and p may be 0; cap may be 0 (`out` may then be NULL): the call sizes. */
mv_status mv_encode_blocks(mv_ctx* ctx, const uint64_t* heads /* n x 10 */, uint32_t n,
                           const uint64_t* includes /* m x 6 */, uint64_t m, const uint8_t* payload_buf,
                           uint64_t payload_bytes, const uint64_t* payload_off /* p */,
                           const uint64_t* payload_len /* p */, uint64_t p, uint32_t flags,
                           const uint8_t* seeds /* n_auth x 32 */, uint32_t n_auth, uint8_t* out, uint64_t cap,
                           uint64_t* out_off /* n */, uint64_t* out_len /* n */, uint8_t* status /* n */,
                           uint64_t* out_bytes, uint8_t* seal_status /* n */, uint8_t* msg_digest /* n x 32 or NULL */,
                           uint8_t* block_digest /* n x 32 or NULL */);
/* mv_encode_blocks with every array in HBM of the context's first device (*out_bytes is the
 * host's). The u64 arrays and d_payload_buf are 8-byte aligned, d_seeds 4-byte; 16 bytes past
 * payload_bytes are readable (payloads are read as whole aligned words); d_out is 8-byte aligned with
 * 16 readable bytes past cap, as mv_dev_seal_blocks asks. The host-buffer call is a copy in, this
 * call and a copy out. Synchronises `stream` once, for the total; without MV_ENCODE_SEAL the bytes are
 * written behind that, in stream order (the next encode call on the context waits for them before it
 * reuses the call's scratch, and reports a bounds check they failed as MV_E_HIP); with it the seal
 * synchronises as mv_dev_seal_blocks does. The image is encoded in d_out before it is sealed there: after
 * MV_E_INVALID_ARG for rounds out of order under MV_ENCODE_LINK d_out holds the encoded blocks with
 * their zero placeholders, unsealed (the host-buffer call does not copy them back), and
 * d_seal_status the seal's first pass. n <= 2^31 - 1, p <= 2^32 - 1. */
mv_status mv_dev_encode_blocks(mv_ctx* ctx, int device, const uint64_t* d_heads, uint32_t n,
                               const uint64_t* d_includes, uint64_t m, const uint8_t* d_payload_buf,
                               uint64_t payload_bytes, const uint64_t* d_payload_off, const uint64_t* d_payload_len,
                               uint64_t p, uint32_t flags, const uint8_t* d_seeds, uint32_t n_auth, uint8_t* d_out,
                               uint64_t cap, uint64_t* d_out_off, uint64_t* d_out_len, uint8_t* d_status,
                               uint64_t* out_bytes, uint8_t* d_seal_status, uint8_t* d_msg_digest,
                               uint8_t* d_block_digest, void* stream);

/* ---- transaction votes: fast-path certificates per block ----
 * What BlockHandler::handle_blocks does with the blocks add_blocks returns (core.rs:171-207,
 * block_handler.rs:146-190): TransactionAggregator::process_block (committee.rs:263-482) over a
 * store in device memory. State is one cell per (sharing block reference B, statement offset o):
 * empty, or aggregating with a voter set and a stake sum. Requires mv_set_committee
 * (MV_E_NO_COMMITTEE) for the stakes and the quorum threshold 2S/3 + 1 (committee.rs:56-57, :79-81).
 *
 * A call processes its blocks in order. For block i (author a, reference R):
 *   1. register (shared_ranges, types.rs:238-254; register, committee.rs:364-384): for every offset
 *      o of block i holding a Share, an empty cell (R, o) becomes aggregating with voters {a} and
 *      stake(a) -- the threshold is not tested here; an aggregating cell is left as it is and the
 *      offset counts as duplicate.
 *   2. vote, in statement order (process_block :463-479, vote :386-425): Vote(locator, Accept) is
 *      the range [o, o + 1) of locator.block, VoteRange [start, end) of its block. For every offset
 *      in ascending order: an empty cell (never registered, certified already, not a Share, past
 *      the block's statements, a block the store has never seen) counts as unknown; otherwise a
 *      joins the voters, its stake is added the first time only, and at a stake sum >= the
 *      threshold the transaction is certified by block i and the cell becomes empty. Share
 *      statements are skipped.
 *   3. a sharing block without an aggregating cell is no longer pending (TransactionAggregator::len
 *      counts the blocks with one).
 * The call does not verify: callers pass blocks that were MV_BLOCK_OK. A block that does not parse
 * (what MV_BLOCK_PARSE_ERROR fails) or whose author is outside the committee changes nothing.
 * Divergences, where the reference has no behaviour to copy: Vote::Reject is unimplemented!()
 * there (committee.rs:472) and a Vote at offset 2^64 - 1 overflows in one(); here each such
 * statement is ignored and its block gets a flag bit. A VoteRange with end < start or
 * end - start >= 2^20 (which verify rejects) counts as empty and is flagged. Blocks with one
 * reference are taken to be one block: Share offsets of a later block at or past the statement
 * count of the first block with that reference are ignored and flagged. */
#define MV_VOTES_OK 0             /* blk_status: processed */
#define MV_VOTES_PARSE_ERROR 1    /* does not deserialize, or its span leaves the buffer: nothing changed */
#define MV_VOTES_UNKNOWN_AUTHOR 2 /* author >= the committee size: nothing changed */
#define MV_VOTES_FLAG_REJECT 1u        /* blk_counts word 3: a Vote::Reject was ignored */
#define MV_VOTES_FLAG_OFFSET 2u        /* a Vote at offset 2^64 - 1 was ignored */
#define MV_VOTES_FLAG_RANGE 4u         /* a VoteRange with end < start or end - start >= 2^20 was ignored */
#define MV_VOTES_FLAG_REF_REUSED 8u    /* Share offsets past the statement count its reference was first seen with */
#define MV_VOTES_REGISTER_ONLY 1u /* flags: step 1 alone -- handle_proposal for the caller's own blocks
                                     (block_handler.rs:199-204) */
/* Makes the store, or grows it, so that `blocks` sharing blocks and `cells` statement offsets fit;
 * never shrinks, keeps what is stored. Opt-in as mv_dag_reserve: the aggregate calls are
 * MV_E_INVALID_ARG without it. The voter set is ceil(committee size / 64) words per cell, fixed
 * here: MV_E_NO_COMMITTEE without a committee; after a committee of another word count
 * mv_votes_clear, then reserve again. The store grows geometrically inside the aggregate calls;
 * rows without an aggregating cell are dropped, and their cells reclaimed, before it would grow
 * and whenever they are half of the cells in use. */
mv_status mv_votes_reserve(mv_ctx* ctx, uint64_t blocks, uint64_t cells);
/* Empties the store and zeroes its counters (capacity and voter word count go too: reserve again). */
mv_status mv_votes_clear(mv_ctx* ctx);
/* out[0] pending sharing blocks (TransactionAggregator::len), out[1] aggregating cells, out[2] cells
 * of capacity in use, out[3] transactions certified since create / clear. */
mv_status mv_votes_stats(mv_ctx* ctx, uint64_t* out /* 4 */);
/* Processes n blocks buf[off[i], off[i] + len[i]) in order (committee.rs:263-482, see above).
 * blk_status[i] = MV_VOTES_*; blk_counts holds four words per block: transactions it certified,
 * unknown offsets, duplicate offsets, MV_VOTES_FLAG_* bits. certified holds 8 words per row: the
 * sharing block's reference in words 0-5 (authority, round, four digest words), the offset in word
 * 6, the index in this call of the certifying block in word 7 -- in the order of the reference's
 * `processed` vectors concatenated: by certifying block, then statement order, then ascending
 * offset. *n_certified is the total; only the first cap_certified rows are written, and the state
 * advances in full whatever the cap (as mv_connect_blocks' `connected`). certified may be NULL with
 * a cap of 0. Runs on the context's first device and takes the context in turn.
 * MV_E_INVALID_ARG (bad arguments, no store, another voter word count) leaves the store as it was.
 * After MV_E_HIP or MV_E_ALLOC the store may hold part of the call: mv_votes_clear. */
mv_status mv_aggregate_votes(mv_ctx* ctx, const uint8_t* buf, const uint64_t* off, const uint64_t* len, uint32_t n,
                             uint32_t flags, uint8_t* blk_status /* n */, uint64_t* blk_counts /* n x 4 */,
                             uint64_t* certified /* cap_certified x 8 */, uint64_t cap_certified,
                             uint64_t* n_certified);

/* ---- device-resident variants (inputs already in HBM of `device`) ----
 * Pointers are device pointers, 16-byte aligned; `stream` is a hipStream_t (NULL = the
 * library's stream for that device). They enqueue work and return without synchronising. */
mv_status mv_dev_ed25519_verify(mv_ctx* ctx, int device, const uint8_t* d_msg, const uint8_t* d_sig,
                                const uint8_t* d_pk, uint32_t n, uint8_t* d_status, void* stream);
/* Batch path on device buffers: verdicts identical to mv_dev_ed25519_verify. The combined
 * equation [8](-[sum z_i s_i]B + sum [z_i]R_i + sum [z_i k_i]A_i) == O with secret random
 * 127-bit z_i (BLAKE2b PRF keyed per context and call) is checked first, per sub-batch group
 * (mv_set_batch_groups); the signatures of every group whose equation fails are re-verified
 * individually on the same stream, so each verdict is exact (an invalid signature survives a
 * passing combination with probability <= 2^-127).
 * `d_pk` rows are indexed by item, or by `d_key_idx` (device array) when it is non-NULL; every
 * d_key_idx[i] must then be a row of d_pk (the library cannot bound-check device arrays).
 * Enqueues only; `d_batch_ok` (optional, device, 4 bytes) receives 1 if the combination held
 * (0 also when dense failures sent the call straight to per-signature verification, see
 * mv_batch_routes). The call makes `stream` wait only for the engine scratch slot it reuses;
 * MV_PREP_CHAIN=2 (mv_set_option) also orders its preparation after the previous call's. */
mv_status mv_dev_ed25519_verify_batch(mv_ctx* ctx, int device, const uint8_t* d_msg, const uint8_t* d_sig,
                                      const uint8_t* d_pk, const uint32_t* d_key_idx, uint32_t n,
                                      uint8_t* d_status, uint32_t* d_batch_ok, void* stream);
mv_status mv_dev_ed25519_sign(mv_ctx* ctx, int device, const uint8_t* d_seed, const uint8_t* d_msg, uint32_t n,
                              uint8_t* d_pk, uint8_t* d_sig, void* stream);
/* StatementBlock::verify on n bincode blocks already in HBM (Data::from_bytes + verify,
 * data.rs:43-52, types.rs:315-376): block i is d_buf[d_off[i] .. d_off[i] + d_len[i]). The
 * parse, the pre-image, both digests, the signature and the committee checks all run on the
 * device; verdicts as mv_verify_blocks. d_buf is 8-byte aligned, blocks do not overlap, and
 * 16 bytes past the end of every block are readable (pad the buffer); buf_bytes bounds the
 * blocks' extent in d_buf. d_msg_digest / d_block_digest (n x 32, 16-byte aligned) may be NULL.
 * Requires mv_set_committee. Enqueue only. */
mv_status mv_dev_verify_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                               const uint64_t* d_off, const uint64_t* d_len, uint32_t n, uint8_t* d_status,
                               uint8_t* d_msg_digest, uint8_t* d_block_digest, void* stream);

/* mv_wal_verify on a WAL image already in HBM (d_wal, 4-byte aligned); outputs are device arrays
 * of `cap` entries and *count is written on the host. Synchronises `stream` (the entry count is
 * data-dependent: the walk's per-map counts come back to the host before the crc pass). */
mv_status mv_dev_wal_verify(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size, uint64_t end_pos,
                            uint32_t map_bits, uint64_t* d_pos, uint32_t* d_tag, uint32_t* d_len, uint8_t* d_status,
                            uint64_t cap, uint64_t* count, void* stream);
/* mv_wal_replay on a WAL image already in HBM (BlockStore::open, block_store.rs:50-116): every array
 * is device memory, d_summary (3 words) and d_last_seen (committee size words) included; *count
 * and *n_blocks are written on the host. d_wal is 8-byte aligned and 16 bytes past `size` are
 * readable (the block path's contract, as mv_dev_verify_blocks; MV_E_INVALID_ARG for a misaligned
 * pointer). Nothing is written past the first min(*count, cap) entries and min(*n_blocks,
 * cap_blocks) rows. Synchronises `stream`, as mv_dev_wal_verify does. */
mv_status mv_dev_wal_replay(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size, uint64_t end_pos,
                            uint32_t map_bits, uint64_t* d_pos, uint32_t* d_tag, uint32_t* d_len, uint8_t* d_status,
                            uint64_t cap, uint64_t* count, uint64_t* d_blk_rows, uint8_t* d_blk_status,
                            uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* d_summary, uint64_t* d_last_seen,
                            void* stream);
/* mv_wal_write with every array in HBM of the context's first device (MV_E_NO_DEVICE for another);
 * *end_pos is written on the host. Payload offsets, lengths and `start` are arbitrary bytes: source
 * and destination need no common alignment. d_buf and d_out follow the block path's contract
 * (mv_dev_verify_blocks): 8-byte aligned, 16 readable bytes past buf_bytes, and the payloads are read
 * where mv_dev_connect_blocks, mv_dev_encode_blocks and mv_dev_seal_blocks leave their blocks -- the
 * offsets and lengths of those calls go into the rows as they are. d_entries and d_pos are 8-byte
 * aligned (MV_E_INVALID_ARG for a misaligned pointer). Synchronises `stream` once, for the checks
 * and the total, like mv_dev_encode_blocks; the bytes are then enqueued behind it, and a bounds
 * check that fails in them is MV_E_HIP from the next WAL write. */
mv_status mv_dev_wal_write(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                           const uint64_t* d_entries /* n x 4 */, uint64_t n, uint64_t start, uint32_t map_bits,
                           uint8_t* d_out, uint64_t cap, uint64_t* d_pos /* n */, uint64_t* end_pos, void* stream);
/* mv_verify_frames on received bytes already in HBM (handle_read_stream, the NetworkMessage decode
 * and process_blocks as there: network.rs:400-457, net_sync.rs:314-383): d_buf, d_soff, d_slen
 * and every output array are device memory; *n_msgs and *n_blocks are written on the host.
 * Synchronises `stream` (the row and block counts depend on the data and size the lists). d_buf is
 * 8-byte aligned and 16 bytes past buf_bytes are readable; a stream that reaches past buf_bytes
 * is clipped to it. Streams whose blocks are verified must not overlap one another (the block
 * path stages a block at its own offset, as mv_dev_verify_blocks). */
mv_status mv_dev_verify_frames(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                               const uint64_t* d_soff, const uint64_t* d_slen, uint32_t ns, uint64_t* d_consumed,
                               uint32_t* d_drop_msg, uint32_t* d_msgs, uint64_t cap_msgs, uint64_t* n_msgs,
                               uint64_t* d_blk_off, uint64_t* d_blk_len, uint8_t* d_blk_status, uint64_t cap_blocks,
                               uint64_t* n_blocks, void* stream);
/* mv_accept_blocks on blocks already in HBM (process_blocks and the lookups of add_blocks as there:
 * net_sync.rs:314-386, block_manager.rs:48-136): every array is device memory (d_grp may be NULL);
 * *n_missing is written on the host. d_buf follows mv_dev_verify_blocks: 8-byte aligned, 16 readable
 * bytes past every block, no overlap. Synchronises `stream` (the counts of blocks to verify and of
 * includes size the lists). It cannot grow the index: MV_E_INDEX_FULL, decided after verify and
 * before the first insert with the index unchanged, when the blocks that are not KNOWN plus the
 * includes of the OK ones may not fit the reserved capacity (mv_index_reserve). */
mv_status mv_dev_accept_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                               const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_grp, uint32_t n,
                               uint8_t* d_blk_status, uint8_t* d_blk_state, uint64_t* d_missing, uint64_t cap_missing,
                               uint64_t* n_missing, void* stream);
/* mv_index_insert of n references that lie in device memory at a stride: reference i is the six words
 * at d_words + i * stride_words (stride_words >= 6); `state` may also be MV_REF_STORED (a replay's
 * rows are stored blocks: a caller of mv_connect_blocks seeds them so). A replay's rows go in straight from HBM
 * (d_blk_rows + 3, stride 10: BlockStore::open's add_unloaded, block_store.rs:398-404). Enqueue only.
 * It cannot grow the index: MV_E_INDEX_FULL, with the index unchanged, when n more entries may not
 * fit. A tag collision (probability 2^-64 per pair at the default MV_INDEX_TAG_BITS) takes more
 * rounds than the call enqueues ahead; it then surfaces as MV_E_HIP from the next index call. */
mv_status mv_dev_index_insert(mv_ctx* ctx, int device, const uint64_t* d_words, uint64_t stride_words, uint64_t n,
                              uint32_t state, void* stream);
/* The seed call of mv_wal_recover (steps 1-3 there: BlockStore::open with add_unloaded, block_store.rs:50-116,
 * 398-404) on the rows of an mv_dev_wal_replay, straight from HBM: d_wal / size are that call's image, d_blk_rows
 * (n_rows x 10 words) and d_blk_status (n_rows) its block rows and their verdicts; `seeded` (5 words) is
 * written on the host. For a caller that uses the DAG store it takes the place of
 * mv_dev_index_insert(d_blk_rows + 3, 10, n_rows, MV_REF_STORED), which raises the references alone.
 * d_wal and d_blk_rows are 8-byte aligned (MV_E_INVALID_ARG otherwise, as mv_dev_wal_replay). A row's
 * offset and length are checked against `size` before a byte is read. Synchronises `stream`: the
 * include total depends on the data. It can grow neither the index nor the DAG store:
 * MV_E_INDEX_FULL, decided before the first insert with index and store unchanged, when n_rows plus
 * the includes of the rows that may get a record may not fit the index at a load of 1/2
 * (mv_index_reserve), or those rows and their includes may not fit the store (mv_dag_reserve).
 * MV_E_NO_COMMITTEE without a committee, MV_E_INVALID_ARG without mv_dag_reserve; n_rows = 0 does
 * nothing. */
mv_status mv_dev_dag_seed_rows(mv_ctx* ctx, int device, const uint8_t* d_wal, uint64_t size,
                               const uint64_t* d_blk_rows /* n_rows x 10 */, const uint8_t* d_blk_status /* n_rows */,
                               uint64_t n_rows, uint64_t floor_round, uint64_t* seeded /* 5, host */, void* stream);
/* mv_connect_blocks on blocks already in HBM, as mv_dev_accept_blocks is to mv_accept_blocks: every
 * array is device memory, *n_missing and *n_connected are written on the host, `stream` is
 * synchronised. It can grow neither the index nor the suspended-block store: MV_E_INDEX_FULL, decided
 * before the first insert with index and store unchanged, when the blocks that are not KNOWN plus the
 * includes of the OK ones may not fit the index (mv_index_reserve) or the store (mv_pending_reserve). */
mv_status mv_dev_connect_blocks(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                                const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_grp, uint32_t n,
                                uint8_t* d_blk_status, uint8_t* d_blk_state, uint64_t* d_missing, uint64_t cap_missing,
                                uint64_t* n_missing, uint64_t* d_connected, uint64_t cap_connected,
                                uint64_t* n_connected, void* stream);
/* mv_decide_leaders with the leader rows and the results in HBM of the context's first device.
 * The rows are read back to be sorted by round; `stream` is synchronised. */
mv_status mv_dev_decide_leaders(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_out,
                                uint64_t* d_stakes /* may be NULL */, void* stream);
/* mv_commit_leaders with the leader rows and the results in HBM of the context's first device;
 * *n_sequence on the host. The rows are read back to be checked and grouped; `stream` is synchronised. */
mv_status mv_dev_commit_leaders(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_out,
                                uint64_t* d_info, uint64_t* n_sequence, void* stream);
/* mv_linearize with the leaders, the blocks and the sub rows in HBM of the context's first device;
 * *n_rows on the host. `stream` is synchronised (the edge counts size the levels' launches). */
mv_status mv_dev_linearize(mv_ctx* ctx, int device, const uint64_t* d_leaders, uint32_t n, uint64_t* d_blocks,
                           uint64_t cap, uint64_t* d_sub, uint64_t* n_rows, void* stream);
/* mv_propose_add (core.rs:181-200, 223-224) with the rows, the tags (may be NULL) and the four result
 * words in HBM of the context's first device: d_rows may be mv_dev_connect_blocks' connected rows as
 * they are (stride 8). `stream` is synchronised (the rows without a slot decide whether anything
 * changes, their rounds size the sort). */
mv_status mv_dev_propose_add(mv_ctx* ctx, int device, const uint64_t* d_rows, uint64_t n, uint64_t stride_words,
                             const uint64_t* d_tags, uint32_t flags, uint64_t payload_token, uint64_t* d_out /* 4 */,
                             void* stream);
/* mv_seal_blocks on blocks already in HBM (new_with_signer as there: types.rs:155-218,
 * crypto.rs:38-61, 199-223): the image is patched in place. Every array is device memory; d_buf is
 * 8-byte aligned with 16 readable bytes past buf_bytes, d_seeds 4-byte and the digest arrays (n x 32,
 * may be NULL) 8-byte aligned. A block whose span leaves buf_bytes is MV_SEAL_PARSE_ERROR.
 * Synchronises `stream` (the call's scratch -- expanded keys, zeroed again before it returns, heads,
 * table -- is the context's, and
 * under MV_SEAL_LINK the order check, the table and the steps come from the heads read back).
 * MV_E_INVALID_ARG for rounds out of order leaves d_buf as it was and d_status holding the first
 * pass's verdicts. The context's first device only. */
mv_status mv_dev_seal_blocks(mv_ctx* ctx, int device, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_off,
                             const uint64_t* d_len, uint32_t n, const uint8_t* d_seeds, uint32_t n_auth,
                             uint32_t flags, uint8_t* d_status, uint8_t* d_msg_digest, uint8_t* d_block_digest,
                             void* stream);
/* mv_aggregate_votes (process_block, committee.rs:263-482) on bincode already in HBM of the
 * context's first device: every array but n_certified is device memory, d_buf 8-byte aligned with 16
 * readable bytes past buf_bytes, the u64 arrays 8-byte aligned. A block whose span leaves buf_bytes is
 * MV_VOTES_PARSE_ERROR. Synchronises `stream` (the scan's totals size the event lists and decide
 * about room). The host-buffer call is a copy in, this call and a copy out. */
mv_status mv_dev_aggregate_votes(mv_ctx* ctx, int device, const uint8_t* d_buf, uint64_t buf_bytes,
                                 const uint64_t* d_off, const uint64_t* d_len, uint32_t n, uint32_t flags,
                                 uint8_t* d_blk_status, uint64_t* d_blk_counts, uint64_t* d_certified,
                                 uint64_t cap_certified, uint64_t* n_certified, void* stream);
/* crc32fast::hash of n strings of device buffer d_buf at d_off/d_len (device arrays) -> d_out. Enqueue only. */
mv_status mv_dev_crc32(mv_ctx* ctx, int device, const uint8_t* d_buf, const uint64_t* d_off, const uint64_t* d_len,
                       uint32_t n, uint32_t* d_out, void* stream);

/* ---- diagnostics (used by the test-suite) ---- */
/* Host-buffer batch-path counters since mv_create: batches tried, batches whose combined
 * equation failed (and were re-verified signature by signature). */
mv_status mv_batch_stats(mv_ctx* ctx, uint64_t* batches, uint64_t* fallbacks);
/* batch counters: out[0] batches, out[1] batches whose combined equation failed in some
 * sub-batch, out[2] sub-batch equations checked, out[3] sub-batch equations that failed
 * (each re-verified signature by signature). Device-API calls are counted once complete. */
mv_status mv_batch_counters(mv_ctx* ctx, uint64_t* out /* 4 */);
/* Routes of batch-path calls under the adaptive policy (config 3, net_sync.rs:352-361: a peer
 * that keeps sending bad signatures): out[0] batches checked by a combined equation (as
 * mv_batch_stats), out[1] batches sent straight to per-signature verification because the
 * failures were dense, out[2] dense failures seen (a guarded batch with at least half of its
 * sub-batch equations failed). Device-API calls are counted once complete. */
mv_status mv_batch_routes(mv_ctx* ctx, uint64_t* out /* 3 */);
/* Sub-batch equations per batch-path call: the batch is cut into groups of whole 1024-signature
 * chunks, each with its own combined equation, and a failed equation re-verifies only its group.
 * groups = 0 (default): adaptive -- 1 group per batch; after a batch whose equation failed,
 * the next 64 batches are cut into 8; after a guarded batch in which at least half of the
 * equations failed (dense failures: the combined check is wasted work), the next batches are
 * verified signature by signature, each counting its invalid signatures, until one holds fewer
 * than 4 (then the guarded equation again). groups = 1..16 fixes the count and disables the
 * dense-failure route. Every call clears the guard. Verdicts never depend on it. */
mv_status mv_set_batch_groups(mv_ctx* ctx, uint32_t groups);
/* Stage timing: when enabled, every call records HIP events on its stream around its
 * stages: batch path 0..5 (prep, sort, bucket, reduce, final, fallback), block pipeline
 * 6..9 (parse, hash, verify = comb/ladder verify when the batch path is not taken, verdict),
 * WAL replay 10..11 (walk = the per-map header walk, crc = the entry crc pass).
 * mv_stage_times waits for the recorded calls and returns the summed device ms per stage and
 * the number of calls measured per stage; reset != 0 clears the sums. */
#define MV_NSTAGES 12
mv_status mv_set_stage_timing(mv_ctx* ctx, int enable);
mv_status mv_stage_times(mv_ctx* ctx, double* ms /* MV_NSTAGES or NULL */, uint64_t* calls /* MV_NSTAGES or NULL */,
                         int reset);
/* Runtime switches (MV_ONLINE, MV_COMB_QUAD, MV_ONLINE_IDLE_US, ...). The library
 * reads every switch from the environment once, at mv_create -- as the reference reads its env
 * knobs at start-up (validator.rs:104-119) -- and never per call. mv_set_option changes one
 * afterwards, between calls (no call on ctx in flight); name is the environment name and value
 * an integer (0 / 1 for on/off switches). Unknown names, and the switches consumed by
 * mv_create (MV_PASS_SETS, MV_GUARD_GROUPS, MV_BASE_GROUPS), are MV_E_INVALID_ARG. No switch
 * changes a verdict, digest or crc. mv_get_option also reads "MV_LIVE_RESOURCES", the
 * process-wide count of live device resources (buffers, events, streams, retired blocks);
 * mv_set_option refuses it. MV_INDEX_TAG_BITS (1..64, default 64) truncates the slot tags of the
 * index from the next mv_index_reserve or mv_index_clear on (tests make tag collisions common). */
mv_status mv_set_option(mv_ctx* ctx, const char* name, int64_t value);
mv_status mv_get_option(mv_ctx* ctx, const char* name, int64_t* value);
/* Runs field/scalar primitive `op` on n lane inputs (16 words each) -> 16 words each (host buffers).
 * Ops >= 64 are the raw-limb field and point test hooks: 64 words in and 64 words out per lane
 * (the row layout is documented at k_selftest_wide in kernels.hip); ops >= 112 call the scalar
 * functions of scalar25519.h on rows of the same width (k_selftest_scalar). */
mv_status mv_selftest(mv_ctx* ctx, int op, const uint32_t* in, uint32_t n, uint32_t* out);
/* Test entry: the preparation stage of the batch path alone (k_bv_prep, batch.hip), launched by
 * the helper the production path launches it with, for n signatures in host arrays (msg, sig and
 * exactly one of pk / key_idx, as mv_ed25519_verify takes them; key_idx needs mv_set_committee).
 * groups: the sub-batch count asked for (clamped as a verify call's). key: 40 bytes, the 32-byte
 * secret of the coefficients z_i and the 64-bit call counter. launch_sigs: 0 = one launch, else a
 * multiple of 256: one launch per launch_sigs signatures, as the chunked copies of pinned inputs
 * gate them. Out (host): scal n x 12 words (z_i in 4, z_i k_i mod l in 8), pts 2 n x 32 words
 * (the affine (y+x, y-x, 2dxy) limb rows of R at i and of A at n + i, 27 words each; with a
 * committee whose A term is summed per key no A row is written: rows n.. stay as they were),
 * bsum 16 x 12 column sums of z_i s_i per group, status n bytes (MV_SIG_* as the preparation
 * decides them), info 3 words: groups, signatures per group, 1 if the A rows were written. The
 * context's call counter, batch counters, guard and route are not touched. */
mv_status mv_selftest_batch_prep(mv_ctx* ctx, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk,
                                 const uint32_t* key_idx, uint32_t n, uint32_t groups, const uint8_t* key,
                                 uint32_t launch_sigs, uint32_t* scal, uint32_t* pts, uint64_t* bsum,
                                 uint8_t* status, uint32_t* info);
/* Test entry: the stages of the batch path between the preparation and the fallback (the sort of
 * the bucket entries, the bucket sums, the per-key A term, the reduction and k_bv_final,
 * batch.hip), launched by the helper the production path launches them with, on rows of the
 * caller's in the layout mv_selftest_batch_prep returns: scal n x 12 words (z < 2^127, z k < 2^253),
 * pts 2 n x 32 words (R at i, A at n + i), bsum 16 x 12 column sums. groups: the sub-batch count
 * asked for. key_idx (optional, with n_keys <= 512 keys of the committee set by mv_set_committee):
 * the per-key form, in which A's term is [sum z k mod l] A_b per key on the committee's tables
 * and only the n R rows of pts are read. Out (host): win 16 x 16 x 36 words, of which groups x nw
 * rows are written, row g * nw + w the extended point (X, Y, Z, T in 9 limbs each) of group g's
 * window w as k_bv_final reads it; asum 16 x 36 words, the groups' per-key A terms (per-key form
 * only); flags 17 words: 1 if every group's equation held, then one per group; info 3 words:
 * groups, signatures per group, nw (16, or 8 in the per-key form). The kernel forms follow the
 * context's options (mv_set_option). No counter, guard or route is touched and no fallback runs. */
mv_status mv_selftest_batch_msm(mv_ctx* ctx, uint32_t n, uint32_t groups, const uint32_t* scal, const uint32_t* pts,
                                const uint64_t* bsum, const uint32_t* key_idx, uint32_t n_keys, uint32_t* win,
                                uint32_t* asum, uint32_t* flags, uint32_t* info);
/* Test entry: reads one radix-256 comb table (comb.h) back from device 0 as it stands: the base
 * point's (key < 0, built by mv_create) or committee key `key`'s (built by mv_set_committee; it
 * holds the multiples of -A). out (host): 32 rows x 129 entries x 32 words (528 KB), entry
 * C[i][j] = [j 256^i]P at words 32 (129 i + j): y+x in words 0..8 (29-bit limbs), y-x in 9..17,
 * 2dxy in 18..26, all canonical, words 27..31 zero. A plain copy after a stream drain: no kernel
 * runs. MV_E_NO_COMMITTEE without a committee, MV_E_INVALID_ARG for a key outside it. The table of
 * a key that does not decode (key_ok 0) is unspecified. */
mv_status mv_selftest_comb_table(mv_ctx* ctx, int key, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MYSTI_VERIFY_H */
