//! Raw declarations of include/mysti_verify.h (the C ABI of libmysti_verify.so).
//! Each entry point names the reference interface it replaces in the header's comments.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

#[repr(C)]
pub struct mv_ctx {
    _p: [u8; 0],
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct mv_config {
    pub device_mask: u32,
    pub max_batch: u32,
    pub flags: u32,
    pub shards_per_device: u32,
}

pub const MV_OK: i32 = 0;
pub const MV_E_INVALID_ARG: i32 = -1;
pub const MV_E_HIP: i32 = -2;
pub const MV_E_NO_DEVICE: i32 = -3;
pub const MV_E_NO_COMMITTEE: i32 = -4;
pub const MV_E_ALLOC: i32 = -5;
pub const MV_E_INDEX_FULL: i32 = -6;

pub const MV_REF_ABSENT: u8 = 0;
pub const MV_REF_WANTED: u8 = 1;
pub const MV_REF_HAVE: u8 = 2;
pub const MV_REF_STORED: u8 = 3;

pub const MV_ACC_REJECTED: u8 = 0;
pub const MV_ACC_NEW: u8 = 1;
pub const MV_ACC_KNOWN: u8 = 2;
pub const MV_ACC_DUP: u8 = 3;
pub const MV_ACC_DROPPED: u8 = 4;
pub const MV_ACC_SUSPENDED: u8 = 5;

pub const MV_LEADER_UNDECIDED: u64 = 0;
pub const MV_LEADER_COMMIT: u64 = 1;
pub const MV_LEADER_SKIP: u64 = 2;
pub const MV_LEADER_CONFLICT: u64 = 3;
pub const MV_LEADER_OVERFLOW: u64 = 4;
pub const MV_DECIDE_MAX_LEADER_BLOCKS: u64 = 8;
pub const MV_COMMIT_KIND_NONE: u64 = 0;
pub const MV_COMMIT_KIND_DIRECT: u64 = 1;
pub const MV_COMMIT_KIND_INDIRECT: u64 = 2;
pub const MV_COMMIT_INCOMPLETE: u64 = 1;
pub const MV_COMMIT_BLOCKED: u64 = 2;
pub const MV_LINEAR_OK: u64 = 0;
pub const MV_LINEAR_INCOMPLETE: u64 = 1;
pub const MV_LINEAR_COMMITTED: u64 = 2;
pub const MV_LINEAR_OVERFLOW: u64 = 3;
pub const MV_LINEAR_STOPPED: u64 = 4;
pub const MV_LINEAR_MAX_DEPTH: u64 = 16;
pub const MV_LINEAR_MAX_INCLUDE: u64 = 65534;
pub const MV_LINEAR_MAX_LEADERS: u64 = 65535;
pub const MV_PROPOSE_IN_ORDER: u32 = 1;
pub const MV_PROPOSE_PAYLOAD: u32 = 2;
pub const MV_PROPOSE_INCOMPLETE: u64 = 1;
pub const MV_PROPOSE_SHORT: u64 = 2;

pub const MV_SIG_OK: u8 = 0;
pub const MV_SIG_INVALID: u8 = 1;
pub const MV_SIG_MALFORMED_KEY: u8 = 2;

pub const MV_BLOCK_OK: u8 = 0;
pub const MV_BLOCK_PARSE_ERROR: u8 = 1;
pub const MV_BLOCK_DIGEST_MISMATCH: u8 = 2;
pub const MV_BLOCK_EPOCH_MISMATCH: u8 = 3;
pub const MV_BLOCK_UNKNOWN_AUTHOR: u8 = 4;
pub const MV_BLOCK_GENESIS: u8 = 5;
pub const MV_BLOCK_SIG_INVALID: u8 = 6;
pub const MV_BLOCK_INCLUDE_UNKNOWN_AUTHORITY: u8 = 7;
pub const MV_BLOCK_INCLUDE_ROUND: u8 = 8;
pub const MV_BLOCK_VOTE_RANGE: u8 = 9;
pub const MV_BLOCK_THRESHOLD_CLOCK: u8 = 10;
pub const MV_BLOCK_VOTE_RANGE_TOO_LONG: u8 = 11;
pub const MV_BLOCK_VOTE_RANGE_END_TOO_LARGE: u8 = 12;

pub const MV_SEAL_OK: u8 = 0;
pub const MV_SEAL_PARSE_ERROR: u8 = 1;
pub const MV_SEAL_UNKNOWN_AUTHOR: u8 = 2;
pub const MV_SEAL_UNLINKED: u8 = 3;
pub const MV_SEAL_LINK: u32 = 1;
pub const MV_ENCODE_OK: u8 = 0;
pub const MV_ENCODE_BAD_HEAD: u8 = 1;
pub const MV_ENCODE_BAD_PAYLOAD: u8 = 2;
pub const MV_ENCODE_TOO_LONG: u8 = 3;
pub const MV_ENCODE_MAX_LEN: u64 = 8388600;
pub const MV_ENCODE_SEAL: u32 = 1;
pub const MV_ENCODE_LINK: u32 = 2;
pub const MV_VOTES_OK: u8 = 0;
pub const MV_VOTES_PARSE_ERROR: u8 = 1;
pub const MV_VOTES_UNKNOWN_AUTHOR: u8 = 2;
pub const MV_VOTES_FLAG_REJECT: u32 = 1;
pub const MV_VOTES_FLAG_OFFSET: u32 = 2;
pub const MV_VOTES_FLAG_RANGE: u32 = 4;
pub const MV_VOTES_FLAG_REF_REUSED: u32 = 8;
pub const MV_VOTES_REGISTER_ONLY: u32 = 1;

pub const MV_WAL_OK: u8 = 0;
pub const MV_WAL_CRC_MISMATCH: u8 = 1;
pub const MV_WAL_NONZERO_CRC_LEN0: u8 = 2;
pub const MV_WAL_BAD_LENGTH: u8 = 3;
pub const MV_WAL_UNKNOWN_TAG: u8 = 4;
pub const MV_WAL_BLOCK_DECODE: u8 = 5;
pub const MV_WAL_UNKNOWN_AUTHORITY: u8 = 6;

pub const MV_MSG_OK: u32 = 0;
pub const MV_MSG_DECODE_ERROR: u32 = 1;
pub const MV_MSG_BLOCK_REJECTED: u32 = 2;
pub const MV_MSG_TOO_MANY_REQUESTED: u32 = 3;
pub const MV_MSG_NOT_REACHED: u32 = 4;
pub const MV_MSG_BAD_SIZE: u32 = 5;

pub const MV_FLAG_NO_BATCH: u32 = 1;
pub const MV_FLAG_NO_COMB: u32 = 2;
pub const MV_FLAG_HOST_PARSE: u32 = 4;
pub const MV_FLAG_NO_ONLINE: u32 = 8;
pub const MV_BATCH_MIN: u32 = 4096;
pub const MV_NSTAGES: usize = 12;

extern "C" {
    pub fn mv_create(cfg: *const mv_config, out: *mut *mut mv_ctx) -> i32;
    pub fn mv_destroy(ctx: *mut mv_ctx);
    pub fn mv_last_error(ctx: *const mv_ctx) -> *const c_char;
    pub fn mv_version() -> *const c_char;
    pub fn mv_set_committee(ctx: *mut mv_ctx, pks: *const u8, stakes: *const u64, n: u32, epoch: u64,
                            key_ok: *mut u8) -> i32;
    pub fn mv_blake2b256(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64, n: u32,
                         out: *mut u8) -> i32;
    pub fn mv_ed25519_verify(ctx: *mut mv_ctx, msg: *const u8, sig: *const u8, pk: *const u8,
                             key_idx: *const u32, n: u32, status: *mut u8) -> i32;
    pub fn mv_host_alloc(ctx: *mut mv_ctx, bytes: u64, out: *mut *mut c_void) -> i32;
    pub fn mv_host_free(ctx: *mut mv_ctx, p: *mut c_void);
    pub fn mv_ed25519_sign(ctx: *mut mv_ctx, seed: *const u8, msg: *const u8, n: u32, pk: *mut u8,
                           sig: *mut u8) -> i32;
    pub fn mv_verify_blocks(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64, n: u32,
                            status: *mut u8, msg_digest: *mut u8, block_digest: *mut u8) -> i32;
    pub fn mv_block_preimage(bincode: *const u8, len: u64, out: *mut u8, cap: u64) -> i64;
    pub fn mv_queue_stats(ctx: *mut mv_ctx, calls: *mut u64, passes: *mut u64) -> i32;
    pub fn mv_online_stats(ctx: *mut mv_ctx, requests: *mut u64, launches: *mut u64) -> i32;
    pub fn mv_shard_plan(weights: *const u64, n: u64, parts: u32, cut: *mut u64) -> i32;
    pub fn mv_crc32(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64, n: u32,
                    out: *mut u32) -> i32;
    pub fn mv_wal_verify(ctx: *mut mv_ctx, wal: *const u8, size: u64, end_pos: u64, map_bits: u32,
                         pos: *mut u64, tag: *mut u32, len: *mut u32, status: *mut u8, cap: u64,
                         count: *mut u64) -> i32;
    pub fn mv_wal_replay(ctx: *mut mv_ctx, wal: *const u8, size: u64, end_pos: u64, map_bits: u32,
                         pos: *mut u64, tag: *mut u32, len: *mut u32, status: *mut u8, cap: u64,
                         count: *mut u64, blk_rows: *mut u64, blk_status: *mut u8, cap_blocks: u64,
                         n_blocks: *mut u64, summary: *mut u64, last_seen: *mut u64) -> i32;
    pub fn mv_wal_recover(ctx: *mut mv_ctx, wal: *const u8, size: u64, end_pos: u64, map_bits: u32,
                          pos: *mut u64, tag: *mut u32, len: *mut u32, status: *mut u8, cap: u64,
                          count: *mut u64, blk_rows: *mut u64, blk_status: *mut u8, cap_blocks: u64,
                          n_blocks: *mut u64, summary: *mut u64, last_seen: *mut u64, floor_round: u64,
                          seeded: *mut u64) -> i32;
    pub fn mv_wal_layout(payload_len: *const u64, n: u64, map_bits: u32, start: u64, pos: *mut u64) -> u64;
    pub fn mv_wal_write(ctx: *mut mv_ctx, buf: *const u8, buf_bytes: u64, entries: *const u64, n: u64, start: u64,
                        map_bits: u32, out: *mut u8, cap: u64, pos: *mut u64, end_pos: *mut u64) -> i32;
    pub fn mv_frame_blocks(buf: *const u8, len: u64, off: *mut u64, blen: *mut u64, cap: u64,
                           consumed: *mut u64) -> i64;
    pub fn mv_frame_messages(buf: *const u8, len: u64, msgs: *mut u32, cap_msgs: u64, blk_off: *mut u64,
                             blk_len: *mut u64, cap_blocks: u64, n_blocks: *mut u64,
                             consumed: *mut u64) -> i64;
    pub fn mv_verify_frames(ctx: *mut mv_ctx, buf: *const u8, soff: *const u64, slen: *const u64, ns: u32,
                            consumed: *mut u64, drop_msg: *mut u32, msgs: *mut u32, cap_msgs: u64,
                            n_msgs: *mut u64, blk_off: *mut u64, blk_len: *mut u64, blk_status: *mut u8,
                            cap_blocks: u64, n_blocks: *mut u64) -> i32;
    pub fn mv_index_reserve(ctx: *mut mv_ctx, entries: u64) -> i32;
    pub fn mv_index_clear(ctx: *mut mv_ctx) -> i32;
    pub fn mv_index_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_index_insert(ctx: *mut mv_ctx, refs: *const u64, n: u64, state: u32, prior: *mut u8) -> i32;
    pub fn mv_index_insert_stored(ctx: *mut mv_ctx, refs: *const u64, n: u64, prior: *mut u8) -> i32;
    pub fn mv_index_lookup(ctx: *mut mv_ctx, refs: *const u64, n: u64, state: *mut u8) -> i32;
    pub fn mv_index_wanted(ctx: *mut mv_ctx, refs: *mut u64, cap: u64, n: *mut u64) -> i32;
    pub fn mv_accept_blocks(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64,
                            grp: *const u64, n: u32, blk_status: *mut u8, blk_state: *mut u8,
                            missing: *mut u64, cap_missing: u64, n_missing: *mut u64) -> i32;
    pub fn mv_dev_accept_blocks(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64,
                                d_off: *const u64, d_len: *const u64, d_grp: *const u64, n: u32,
                                d_blk_status: *mut u8, d_blk_state: *mut u8, d_missing: *mut u64,
                                cap_missing: u64, n_missing: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_connect_blocks(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64,
                             grp: *const u64, n: u32, blk_status: *mut u8, blk_state: *mut u8,
                             missing: *mut u64, cap_missing: u64, n_missing: *mut u64,
                             connected: *mut u64, cap_connected: u64, n_connected: *mut u64) -> i32;
    pub fn mv_dev_connect_blocks(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64,
                                 d_off: *const u64, d_len: *const u64, d_grp: *const u64, n: u32,
                                 d_blk_status: *mut u8, d_blk_state: *mut u8, d_missing: *mut u64,
                                 cap_missing: u64, n_missing: *mut u64, d_connected: *mut u64,
                                 cap_connected: u64, n_connected: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_pending_reserve(ctx: *mut mv_ctx, blocks: u64, includes: u64) -> i32;
    pub fn mv_pending_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_dag_reserve(ctx: *mut mv_ctx, blocks: u64, includes: u64) -> i32;
    pub fn mv_dag_prune(ctx: *mut mv_ctx, round: u64) -> i32;
    pub fn mv_dag_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_decide_leaders(ctx: *mut mv_ctx, leaders: *const u64, n: u32, out: *mut u64, stakes: *mut u64) -> i32;
    pub fn mv_dev_decide_leaders(ctx: *mut mv_ctx, device: i32, d_leaders: *const u64, n: u32, d_out: *mut u64,
                                 d_stakes: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_commit_leaders(ctx: *mut mv_ctx, leaders: *const u64, n: u32, out: *mut u64, info: *mut u64,
                             n_sequence: *mut u64) -> i32;
    pub fn mv_dev_commit_leaders(ctx: *mut mv_ctx, device: i32, d_leaders: *const u64, n: u32, d_out: *mut u64,
                                 d_info: *mut u64, n_sequence: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_linearize(ctx: *mut mv_ctx, leaders: *const u64, n: u32, blocks: *mut u64, cap: u64, sub: *mut u64,
                        n_rows: *mut u64) -> i32;
    pub fn mv_dev_linearize(ctx: *mut mv_ctx, device: i32, d_leaders: *const u64, n: u32, d_blocks: *mut u64, cap: u64,
                            d_sub: *mut u64, n_rows: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_linearize_mark(ctx: *mut mv_ctx, refs: *const u64, n: u64, height: u64) -> i32;
    pub fn mv_linearize_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_propose_reserve(ctx: *mut mv_ctx, authority: u32, entries: u64) -> i32;
    pub fn mv_propose_add(ctx: *mut mv_ctx, rows: *const u64, n: u64, stride_words: u64, tags: *const u64, flags: u32,
                          payload_token: u64, out: *mut u64) -> i32;
    pub fn mv_dev_propose_add(ctx: *mut mv_ctx, device: i32, d_rows: *const u64, n: u64, stride_words: u64,
                              d_tags: *const u64, flags: u32, payload_token: u64, d_out: *mut u64,
                              stream: *mut c_void) -> i32;
    pub fn mv_propose_take(ctx: *mut mv_ctx, includes: *mut u64, cap: u64, n_includes: *mut u64, payloads: *mut u64,
                           cap_p: u64, n_payloads: *mut u64, out: *mut u64) -> i32;
    pub fn mv_propose_own(ctx: *mut mv_ctx, block_ref: *const u64, includes: *const u64, k: u64, out: *mut u64) -> i32;
    pub fn mv_propose_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_dev_index_insert(ctx: *mut mv_ctx, device: i32, d_words: *const u64, stride_words: u64, n: u64,
                               state: u32, stream: *mut c_void) -> i32;
    pub fn mv_dev_dag_seed_rows(ctx: *mut mv_ctx, device: i32, d_wal: *const u8, size: u64, d_blk_rows: *const u64,
                                d_blk_status: *const u8, n_rows: u64, floor_round: u64, seeded: *mut u64,
                                stream: *mut c_void) -> i32;
    pub fn mv_seal_blocks(ctx: *mut mv_ctx, buf: *mut u8, off: *const u64, len: *const u64, n: u32,
                          seeds: *const u8, n_auth: u32, flags: u32, status: *mut u8, msg_digest: *mut u8,
                          block_digest: *mut u8) -> i32;
    pub fn mv_dev_seal_blocks(ctx: *mut mv_ctx, device: i32, d_buf: *mut u8, buf_bytes: u64, d_off: *const u64,
                              d_len: *const u64, n: u32, d_seeds: *const u8, n_auth: u32, flags: u32,
                              d_status: *mut u8, d_msg_digest: *mut u8, d_block_digest: *mut u8,
                              stream: *mut c_void) -> i32;
    pub fn mv_encode_blocks(ctx: *mut mv_ctx, heads: *const u64, n: u32, includes: *const u64, m: u64,
                            payload_buf: *const u8, payload_bytes: u64, payload_off: *const u64,
                            payload_len: *const u64, p: u64, flags: u32, seeds: *const u8, n_auth: u32,
                            out: *mut u8, cap: u64, out_off: *mut u64, out_len: *mut u64, status: *mut u8,
                            out_bytes: *mut u64, seal_status: *mut u8, msg_digest: *mut u8,
                            block_digest: *mut u8) -> i32;
    pub fn mv_dev_encode_blocks(ctx: *mut mv_ctx, device: i32, d_heads: *const u64, n: u32, d_includes: *const u64,
                                m: u64, d_payload_buf: *const u8, payload_bytes: u64, d_payload_off: *const u64,
                                d_payload_len: *const u64, p: u64, flags: u32, d_seeds: *const u8, n_auth: u32,
                                d_out: *mut u8, cap: u64, d_out_off: *mut u64, d_out_len: *mut u64,
                                d_status: *mut u8, out_bytes: *mut u64, d_seal_status: *mut u8,
                                d_msg_digest: *mut u8, d_block_digest: *mut u8, stream: *mut c_void) -> i32;
    pub fn mv_votes_reserve(ctx: *mut mv_ctx, blocks: u64, cells: u64) -> i32;
    pub fn mv_votes_clear(ctx: *mut mv_ctx) -> i32;
    pub fn mv_votes_stats(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_aggregate_votes(ctx: *mut mv_ctx, buf: *const u8, off: *const u64, len: *const u64, n: u32,
                              flags: u32, blk_status: *mut u8, blk_counts: *mut u64, certified: *mut u64,
                              cap_certified: u64, n_certified: *mut u64) -> i32;
    pub fn mv_dev_aggregate_votes(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64,
                                  d_off: *const u64, d_len: *const u64, n: u32, flags: u32,
                                  d_blk_status: *mut u8, d_blk_counts: *mut u64, d_certified: *mut u64,
                                  cap_certified: u64, n_certified: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_dev_verify_frames(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64,
                                d_soff: *const u64, d_slen: *const u64, ns: u32, d_consumed: *mut u64,
                                d_drop_msg: *mut u32, d_msgs: *mut u32, cap_msgs: u64, n_msgs: *mut u64,
                                d_blk_off: *mut u64, d_blk_len: *mut u64, d_blk_status: *mut u8,
                                cap_blocks: u64, n_blocks: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_dev_ed25519_verify(ctx: *mut mv_ctx, device: i32, d_msg: *const u8, d_sig: *const u8,
                                 d_pk: *const u8, n: u32, d_status: *mut u8, stream: *mut c_void) -> i32;
    pub fn mv_dev_ed25519_verify_batch(ctx: *mut mv_ctx, device: i32, d_msg: *const u8, d_sig: *const u8,
                                       d_pk: *const u8, d_key_idx: *const u32, n: u32, d_status: *mut u8,
                                       d_batch_ok: *mut u32, stream: *mut c_void) -> i32;
    pub fn mv_dev_ed25519_sign(ctx: *mut mv_ctx, device: i32, d_seed: *const u8, d_msg: *const u8, n: u32,
                               d_pk: *mut u8, d_sig: *mut u8, stream: *mut c_void) -> i32;
    pub fn mv_dev_verify_blocks(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64,
                                d_off: *const u64, d_len: *const u64, n: u32, d_status: *mut u8,
                                d_msg_digest: *mut u8, d_block_digest: *mut u8, stream: *mut c_void) -> i32;
    pub fn mv_dev_wal_verify(ctx: *mut mv_ctx, device: i32, d_wal: *const u8, size: u64, end_pos: u64,
                             map_bits: u32, d_pos: *mut u64, d_tag: *mut u32, d_len: *mut u32,
                             d_status: *mut u8, cap: u64, count: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_dev_wal_replay(ctx: *mut mv_ctx, device: i32, d_wal: *const u8, size: u64, end_pos: u64,
                             map_bits: u32, d_pos: *mut u64, d_tag: *mut u32, d_len: *mut u32,
                             d_status: *mut u8, cap: u64, count: *mut u64, d_blk_rows: *mut u64,
                             d_blk_status: *mut u8, cap_blocks: u64, n_blocks: *mut u64,
                             d_summary: *mut u64, d_last_seen: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_dev_wal_write(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, buf_bytes: u64, d_entries: *const u64,
                            n: u64, start: u64, map_bits: u32, d_out: *mut u8, cap: u64, d_pos: *mut u64,
                            end_pos: *mut u64, stream: *mut c_void) -> i32;
    pub fn mv_dev_crc32(ctx: *mut mv_ctx, device: i32, d_buf: *const u8, d_off: *const u64, d_len: *const u64,
                        n: u32, d_out: *mut u32, stream: *mut c_void) -> i32;
    pub fn mv_batch_stats(ctx: *mut mv_ctx, batches: *mut u64, fallbacks: *mut u64) -> i32;
    pub fn mv_batch_counters(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_batch_routes(ctx: *mut mv_ctx, out: *mut u64) -> i32;
    pub fn mv_set_batch_groups(ctx: *mut mv_ctx, groups: u32) -> i32;
    pub fn mv_set_stage_timing(ctx: *mut mv_ctx, enable: i32) -> i32;
    pub fn mv_stage_times(ctx: *mut mv_ctx, ms: *mut f64, calls: *mut u64, reset: i32) -> i32;
    pub fn mv_selftest(ctx: *mut mv_ctx, op: i32, input: *const u32, n: u32, out: *mut u32) -> i32;
    pub fn mv_selftest_batch_prep(ctx: *mut mv_ctx, msg: *const u8, sig: *const u8, pk: *const u8,
                                  key_idx: *const u32, n: u32, groups: u32, key: *const u8, launch_sigs: u32,
                                  scal: *mut u32, pts: *mut u32, bsum: *mut u64, status: *mut u8,
                                  info: *mut u32) -> i32;
    pub fn mv_selftest_batch_msm(ctx: *mut mv_ctx, n: u32, groups: u32, scal: *const u32, pts: *const u32,
                                 bsum: *const u64, key_idx: *const u32, n_keys: u32, win: *mut u32,
                                 asum: *mut u32, flags: *mut u32, info: *mut u32) -> i32;
    pub fn mv_selftest_comb_table(ctx: *mut mv_ctx, key: i32, out: *mut u32) -> i32;
    pub fn mv_set_option(ctx: *mut mv_ctx, name: *const c_char, value: i64) -> i32;
    pub fn mv_get_option(ctx: *mut mv_ctx, name: *const c_char, value: *mut i64) -> i32;
}
