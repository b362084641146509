"""mysticeti_amd — MI355X (gfx950) StatementBlock verification engine.

Python host binding of libmysti_verify.so (C ABI: include/mysti_verify.h). The
GPU path is the only path: importing works without a GPU, but every compute call
goes through the HIP library and raises if it (or a device) is missing — there is
no CPU fallback.

Reference interfaces mirrored (hrubaanna/mysticeti @ 2025-02-04):
  Engine.verify_blocks     NetworkSyncer::process_blocks' per-block StatementBlock::verify
                           (net_sync.rs:331-375, types.rs:315-376)
  Engine.ed25519_verify    PublicKey::verify_block -> VerificationKey::verify (crypto.rs:174-189)
  Engine.ed25519_sign      Signer::sign_block (crypto.rs:199-223)
  Engine.blake2b256        BlockHasher (crypto.rs:34)
  Engine.crc32             crc32fast::hash as the WAL uses it (wal.rs:173-177, :250)
  Engine.wal_verify        WalReader::iter_until / WalIterator over try_read (wal.rs:226-346)
  Engine.wal_replay        the replay loop of BlockStore::open (block_store.rs:50-116): entries, one
                           row per decoded block with its verify status, highest_round,
                           last_seen_by_authority
  Engine.dev_wal_replay    the same on an image already in HBM
  Engine.wal_iter_until    the same as the reference's iterator: (pos, (tag, bytes)), raising
                           where the reference panics
  wal_layout               WalWriter::writev positions (wal.rs:150-188)
  Engine.wal_write (and dev_wal_write)
                           WalWriter::writev for many entries (wal.rs:150-188, 211-216), as
                           BlockWriter::insert_block and OwnBlockData::write_to_wal use it
                           (block_store.rs:504-518, 542-549): the appended bytes and the positions
  Engine.verify_frames_messages
                           what a connection does with its received bytes, per message:
                           handle_read_stream + the NetworkMessage decode (network.rs:400-457) and
                           process_blocks (net_sync.rs:314-383), for many connections at once
  Engine.dev_verify_frames the same on bytes already in HBM
  Engine.index_*           the BlockReferences the core answers from, in device memory:
                           BlockManager::exists_or_pending and ::missing (block_manager.rs:26, 138-144)
  Engine.accept_blocks     process_blocks with its `processed` skip ahead of verify (net_sync.rs:325-336)
                           and the include lookups of BlockManager::add_blocks after it
                           (block_manager.rs:48-136): per-block outcomes and the missing references
  Engine.connect_blocks    accept_blocks and the suspend / unlock cascade of add_blocks
                           (block_manager.rs:102-131) over a store of suspended blocks in device memory:
                           the blocks the core may process, in a causal order
  Engine.dag_reserve, Engine.dag_prune, Engine.dag_stats, Engine.decide_leaders (and dev_decide_leaders)
                           the edges of the blocks connect_blocks stored, kept on the GPU, and
                           BaseCommitter::try_direct_decide over them (base_committer.rs:323-357)
  Engine.commit_leaders (and dev_commit_leaders)
                           UniversalCommitter::try_commit over them (universal_committer.rs:30-90): the direct
                           rule, try_indirect_decide (base_committer.rs:294-318) and the decided prefix
  Engine.linearize (and dev_linearize, linearize_mark, linearize_stats)
                           Linearizer::handle_commit (linearizer.rs:125-166): the committed leaders' sub-DAGs in
                           the reference's order, with the committed marks and last_height kept in the engine
  Engine.propose_reserve, propose_add (and dev_propose_add), propose_take, propose_own, propose_stats
                           the threshold clock (threshold_clock.rs:58-89), Core's `pending` queue and the include
                           choice of Core::try_new_block (core.rs:181-278), with the own block's DAG record
  Engine.dev_accept_blocks, Engine.dev_connect_blocks, Engine.dev_index_insert
                           the same on buffers already in HBM (a replay's rows go in at a stride)
  frame_messages           the frame and message walk alone, on the host, for one stream
  crypto.*                 thin reference-named wrappers (BlockDigest, PublicKey, Signer, ...)
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import os
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MV_LIB selects an experiment build (python -m mysticeti_amd.build --variant NAME -D...)
LIB_PATH = os.environ.get("MV_LIB") or os.path.join(_HERE, "libmysti_verify.so")

MV_OK = 0
SIG_OK, SIG_INVALID, SIG_MALFORMED_KEY = 0, 1, 2
BLOCK_STATUS = [
    "OK", "PARSE_ERROR", "DIGEST_MISMATCH", "EPOCH_MISMATCH", "UNKNOWN_AUTHOR", "GENESIS", "SIG_INVALID",
    "INCLUDE_UNKNOWN_AUTHORITY", "INCLUDE_ROUND", "VOTE_RANGE", "THRESHOLD_CLOCK", "VOTE_RANGE_TOO_LONG",
    "VOTE_RANGE_END_TOO_LARGE",
]
(BLOCK_OK, BLOCK_PARSE_ERROR, BLOCK_DIGEST_MISMATCH, BLOCK_EPOCH_MISMATCH, BLOCK_UNKNOWN_AUTHOR,
 BLOCK_GENESIS, BLOCK_SIG_INVALID, BLOCK_INCLUDE_UNKNOWN_AUTHORITY, BLOCK_INCLUDE_ROUND,
 BLOCK_VOTE_RANGE, BLOCK_THRESHOLD_CLOCK, BLOCK_VOTE_RANGE_TOO_LONG, BLOCK_VOTE_RANGE_END_TOO_LARGE) = range(13)

EXPORTS = [
    "mv_create", "mv_destroy", "mv_last_error", "mv_version", "mv_set_committee", "mv_blake2b256",
    "mv_ed25519_verify", "mv_ed25519_sign", "mv_verify_blocks", "mv_dev_ed25519_verify",
    "mv_dev_ed25519_sign", "mv_selftest", "mv_selftest_batch_prep", "mv_selftest_batch_msm", "mv_selftest_comb_table", "mv_block_preimage", "mv_dev_ed25519_verify_batch", "mv_batch_stats",
    "mv_set_stage_timing", "mv_stage_times", "mv_dev_verify_blocks", "mv_batch_counters", "mv_batch_routes", "mv_set_batch_groups",
    "mv_queue_stats", "mv_shard_plan", "mv_crc32", "mv_wal_verify", "mv_wal_layout", "mv_dev_wal_verify",
    "mv_frame_blocks", "mv_frame_messages", "mv_verify_frames", "mv_dev_verify_frames",
    "mv_index_reserve", "mv_index_clear", "mv_index_stats", "mv_index_insert", "mv_index_lookup", "mv_index_wanted",
    "mv_accept_blocks", "mv_dev_accept_blocks", "mv_dev_index_insert",
    "mv_index_insert_stored", "mv_connect_blocks", "mv_dev_connect_blocks", "mv_pending_reserve", "mv_pending_stats",
    "mv_dag_reserve", "mv_dag_prune", "mv_dag_stats", "mv_decide_leaders", "mv_dev_decide_leaders",
    "mv_commit_leaders", "mv_dev_commit_leaders", "mv_wal_recover", "mv_dev_dag_seed_rows",
    "mv_linearize", "mv_dev_linearize", "mv_linearize_mark", "mv_linearize_stats",
    "mv_propose_reserve", "mv_propose_add", "mv_dev_propose_add", "mv_propose_take", "mv_propose_own", "mv_propose_stats",
    "mv_seal_blocks", "mv_dev_seal_blocks", "mv_encode_blocks", "mv_dev_encode_blocks",
    "mv_votes_reserve", "mv_votes_clear", "mv_votes_stats", "mv_aggregate_votes", "mv_dev_aggregate_votes",
    "mv_wal_write", "mv_dev_wal_write",
    "mv_wal_replay", "mv_dev_wal_replay", "mv_dev_crc32", "mv_host_alloc", "mv_host_free", "mv_online_stats", "mv_set_option", "mv_get_option",
]
# per-block outcomes of mv_seal_blocks, and its flag
SEAL_STATUS = ["OK", "PARSE_ERROR", "UNKNOWN_AUTHOR", "UNLINKED"]
SEAL_OK, SEAL_PARSE_ERROR, SEAL_UNKNOWN_AUTHOR, SEAL_UNLINKED = range(4)
SEAL_LINK = 1
# per-block outcomes of mv_encode_blocks, its length limit (wal.rs:107: MAX_ENTRY_SIZE / 2), its flags and the
# words of a head row
ENCODE_STATUS = ["OK", "BAD_HEAD", "BAD_PAYLOAD", "TOO_LONG"]
ENCODE_OK, ENCODE_BAD_HEAD, ENCODE_BAD_PAYLOAD, ENCODE_TOO_LONG = range(4)
ENCODE_MAX_LEN = 8388600
ENCODE_SEAL, ENCODE_LINK = 1, 2
ENCODE_HEAD_WORDS = 10
# per-block outcomes of mv_aggregate_votes, the flag bits of a block's fourth count word, the call's flag
VOTES_STATUS = ["OK", "PARSE_ERROR", "UNKNOWN_AUTHOR"]
VOTES_OK, VOTES_PARSE_ERROR, VOTES_UNKNOWN_AUTHOR = range(3)
VOTES_FLAG_REJECT, VOTES_FLAG_OFFSET, VOTES_FLAG_RANGE, VOTES_FLAG_REF_REUSED = 1, 2, 4, 8
VOTES_REGISTER_ONLY = 1
WAL_OK, WAL_CRC_MISMATCH, WAL_NONZERO_CRC_LEN0, WAL_BAD_LENGTH = range(4)
# ... and of the replay loop of BlockStore::open (mv_wal_replay only)
WAL_UNKNOWN_TAG, WAL_BLOCK_DECODE, WAL_UNKNOWN_AUTHORITY = 4, 5, 6
WAL_NONE = 0xFFFFFFFFFFFFFFFF  # mv_wal_replay: no such row / entry, next_entry of a tag-1 row
WAL_ROW_WORDS = 10
# per-message verdicts (mv_verify_frames rows, word 6's low byte) and the rows' "none" word
MSG_STATUS = ["OK", "DECODE_ERROR", "BLOCK_REJECTED", "TOO_MANY_REQUESTED", "NOT_REACHED", "BAD_SIZE"]
MSG_OK, MSG_DECODE_ERROR, MSG_BLOCK_REJECTED, MSG_TOO_MANY_REQUESTED, MSG_NOT_REACHED, MSG_BAD_SIZE = range(6)
MSG_NONE = 0xFFFFFFFF
# the index of block references: states of a reference, per-block outcomes of accept_blocks
REF_ABSENT, REF_WANTED, REF_HAVE, REF_STORED = 0, 1, 2, 3
ACC_STATE = ["REJECTED", "NEW", "KNOWN", "DUP", "DROPPED", "SUSPENDED"]
ACC_REJECTED, ACC_NEW, ACC_KNOWN, ACC_DUP, ACC_DROPPED, ACC_SUSPENDED = range(6)
CONNECT_EARLIER = 0xFFFFFFFFFFFFFFFF  # word 6 of a connected row: an earlier call suspended the block
E_INDEX_FULL = -6
E_INVALID_ARG, E_NO_COMMITTEE = -1, -4
# mv_decide_leaders: word 6 of a row, and the leader blocks a row can tell apart
LEADER_STATUS = ["UNDECIDED", "COMMIT", "SKIP", "CONFLICT", "OVERFLOW"]
LEADER_UNDECIDED, LEADER_COMMIT, LEADER_SKIP, LEADER_CONFLICT, LEADER_OVERFLOW = range(5)
DECIDE_MAX_LEADER_BLOCKS = 8
# mv_commit_leaders: word 0 of an info row, the bits of word 2, word 1 without an anchor
COMMIT_KIND_NONE, COMMIT_KIND_DIRECT, COMMIT_KIND_INDIRECT = range(3)
COMMIT_INCOMPLETE, COMMIT_BLOCKED = 1, 2
COMMIT_NO_ANCHOR = 0xFFFFFFFFFFFFFFFF
# mv_linearize: word 0 of a sub row, and the limits of a path
LINEAR_STATUS = ["OK", "INCOMPLETE", "COMMITTED", "OVERFLOW", "STOPPED"]
LINEAR_OK, LINEAR_INCOMPLETE, LINEAR_COMMITTED, LINEAR_OVERFLOW, LINEAR_STOPPED = range(5)
LINEAR_MAX_DEPTH, LINEAR_MAX_INCLUDE, LINEAR_MAX_LEADERS = 16, 0xFFFE, 0xFFFF
# mv_propose_add's flags, the flag bits of mv_propose_take's out[3], its out[4] without an entry left
PROPOSE_IN_ORDER, PROPOSE_PAYLOAD = 1, 2
PROPOSE_INCOMPLETE, PROPOSE_SHORT = 1, 2
PROPOSE_NO_ENTRY = 0xFFFFFFFFFFFFFFFF
PROPOSE_GUARD = 0xA5A5A5A5A5A5A5A5  # Engine.propose_take: what stands behind cap rows before the call
WAL_MAP_BITS, WAL_MAP_BITS_TEST = 24, 16  # wal.rs:95-103
# batch path stages, the block pipeline's, the WAL replay's (mv_stage_times order, MV_NSTAGES)
STAGES = ["prep", "sort", "bucket", "reduce", "final", "fallback", "parse", "hash", "verify", "verdict", "wal_walk",
          "wal_crc"]
FLAG_NO_BATCH, FLAG_NO_COMB, FLAG_HOST_PARSE, FLAG_NO_ONLINE = 1, 2, 4, 8
BATCH_MIN = 4096
SELFTEST_WIDE_OP = 64  # mv_selftest ops from here on use 64-word rows
BATCH_MAX_GROUPS = 16  # sub-batch equations per batch at most
COMB_ROWS, COMB_ENTRIES = 32, 129  # a comb table (csrc/comb.h): radix-256 digit positions, |digit| 0..128
BATCH_PREP_UNWRITTEN = 0xA5A5A5A5  # Engine.batch_prep: the words of point rows that were not read back


class MvError(RuntimeError):
    """A failed library call; `code` is the MV_E_* status when there is one."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class EncodeResult(NamedTuple):
    """Engine.encode_blocks: the image, where each block starts and how long it is, MV_ENCODE_* per
    block, the whole span; with seal=True MV_SEAL_* per block and both digests, else None."""
    buf: np.ndarray
    offs: np.ndarray
    lens: np.ndarray
    status: np.ndarray
    out_bytes: int
    seal_status: Optional[np.ndarray]
    msg_digest: Optional[np.ndarray]
    block_digest: Optional[np.ndarray]


def encode_bound(heads: np.ndarray, m: int, payload_len: np.ndarray) -> int:
    """An upper bound of mv_encode_blocks' *out_bytes from the heads and the payload lengths alone: a
    head whose runs are inside gives 176 + 56 k + the lengths of its payloads, any other nothing."""
    heads = np.asarray(heads, dtype=np.uint64).reshape(-1, ENCODE_HEAD_WORDS)
    if heads.shape[0] == 0:
        return 0
    p = int(payload_len.shape[0])
    cum = np.zeros(p + 1, dtype=np.float64)
    cum[1:] = np.cumsum(payload_len.astype(np.float64))
    inc0, k, pay0, np_ = (heads[:, w].astype(np.float64) for w in (6, 7, 8, 9))
    ok = (inc0 + k <= m) & (pay0 + np_ <= p)
    lo = np.where(ok, pay0, 0).astype(np.int64)
    hi = np.where(ok, pay0 + np_, 0).astype(np.int64)
    size = np.where(ok, 176 + 56 * k + cum[hi] - cum[lo], 0)
    size = np.minimum(size, ENCODE_MAX_LEN + 8)
    return int(size.sum())


class _Config(ctypes.Structure):
    _fields_ = [("device_mask", ctypes.c_uint32), ("max_batch", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("shards_per_device", ctypes.c_uint32)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load libmysti_verify.so (in-tree). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise MvError(f"{path} missing: build it with `python -m mysticeti_amd.build` (no CPU fallback exists)")
    lib = ctypes.CDLL(path)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.mv_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(vp)]
    lib.mv_destroy.argtypes = [vp]
    lib.mv_destroy.restype = None
    lib.mv_last_error.argtypes = [vp]
    lib.mv_last_error.restype = ctypes.c_char_p
    lib.mv_version.restype = ctypes.c_char_p
    lib.mv_set_committee.argtypes = [vp, vp, vp, u32, u64, vp]
    lib.mv_blake2b256.argtypes = [vp, vp, vp, vp, u32, vp]
    lib.mv_ed25519_verify.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    lib.mv_ed25519_sign.argtypes = [vp, vp, vp, u32, vp, vp]
    lib.mv_verify_blocks.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
    lib.mv_dev_ed25519_verify.argtypes = [vp, ctypes.c_int, vp, vp, vp, u32, vp, vp]
    lib.mv_dev_ed25519_verify_batch.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.mv_batch_stats.argtypes = [vp, vp, vp]
    lib.mv_batch_counters.argtypes = [vp, vp]
    lib.mv_batch_routes.argtypes = [vp, vp]
    lib.mv_set_batch_groups.argtypes = [vp, u32]
    lib.mv_queue_stats.argtypes = [vp, vp, vp]
    lib.mv_online_stats.argtypes = [vp, vp, vp]
    lib.mv_shard_plan.argtypes = [vp, u64, u32, vp]
    lib.mv_set_stage_timing.argtypes = [vp, ctypes.c_int]
    lib.mv_stage_times.argtypes = [vp, vp, vp, ctypes.c_int]
    lib.mv_dev_verify_blocks.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, u32, vp, vp, vp, vp]
    lib.mv_dev_ed25519_sign.argtypes = [vp, ctypes.c_int, vp, vp, u32, vp, vp, vp]
    lib.mv_seal_blocks.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    lib.mv_dev_seal_blocks.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp]
    lib.mv_encode_blocks.argtypes = [vp, vp, u32, vp, u64, vp, u64, vp, vp, u64, u32, vp, u32, vp, u64, vp, vp, vp, vp,
                                     vp, vp, vp]
    lib.mv_dev_encode_blocks.argtypes = [vp, ctypes.c_int, vp, u32, vp, u64, vp, u64, vp, vp, u64, u32, vp, u32, vp, u64,
                                         vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mv_votes_reserve.argtypes = [vp, u64, u64]
    lib.mv_votes_clear.argtypes = [vp]
    lib.mv_votes_stats.argtypes = [vp, vp]
    lib.mv_aggregate_votes.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, vp]
    lib.mv_dev_aggregate_votes.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, u32, u32, vp, vp, vp, u64, vp, vp]
    lib.mv_selftest.argtypes = [vp, ctypes.c_int, vp, u32, vp]
    lib.mv_selftest_batch_prep.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp]
    lib.mv_selftest_batch_msm.argtypes = [vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.mv_selftest_comb_table.argtypes = [vp, ctypes.c_int, vp]
    lib.mv_block_preimage.argtypes = [vp, u64, vp, u64]
    lib.mv_block_preimage.restype = ctypes.c_int64
    lib.mv_crc32.argtypes = [vp, vp, vp, vp, u32, vp]
    lib.mv_wal_verify.argtypes = [vp, vp, u64, u64, u32, vp, vp, vp, vp, u64, vp]
    lib.mv_wal_layout.argtypes = [vp, u64, u32, u64, vp]
    lib.mv_wal_layout.restype = u64
    lib.mv_wal_write.argtypes = [vp, vp, u64, vp, u64, u64, u32, vp, u64, vp, vp]
    lib.mv_dev_wal_write.argtypes = [vp, ctypes.c_int, vp, u64, vp, u64, u64, u32, vp, u64, vp, vp, vp]
    lib.mv_frame_blocks.argtypes = [vp, u64, vp, vp, u64, vp]
    lib.mv_frame_blocks.restype = ctypes.c_int64
    lib.mv_frame_messages.argtypes = [vp, u64, vp, u64, vp, vp, u64, vp, vp]
    lib.mv_frame_messages.restype = ctypes.c_int64
    lib.mv_verify_frames.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]
    lib.mv_dev_verify_frames.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64,
                                         vp, vp]
    lib.mv_dev_wal_verify.argtypes = [vp, ctypes.c_int, vp, u64, u64, u32, vp, vp, vp, vp, u64, vp, vp]
    lib.mv_wal_replay.argtypes = [vp, vp, u64, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp]
    lib.mv_dev_wal_replay.argtypes = [vp, ctypes.c_int, vp, u64, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp,
                                      vp, vp]
    lib.mv_wal_recover.argtypes = [vp, vp, u64, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, vp]
    lib.mv_dev_dag_seed_rows.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, u64, u64, vp, vp]
    lib.mv_dev_crc32.argtypes = [vp, ctypes.c_int, vp, vp, vp, u32, vp, vp]
    lib.mv_index_reserve.argtypes = [vp, u64]
    lib.mv_index_clear.argtypes = [vp]
    lib.mv_index_stats.argtypes = [vp, vp]
    lib.mv_index_insert.argtypes = [vp, vp, u64, u32, vp]
    lib.mv_index_lookup.argtypes = [vp, vp, u64, vp]
    lib.mv_index_wanted.argtypes = [vp, vp, u64, vp]
    lib.mv_accept_blocks.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, u64, vp]
    lib.mv_dev_accept_blocks.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, vp, u32, vp, vp, vp, u64, vp, vp]
    lib.mv_dev_index_insert.argtypes = [vp, ctypes.c_int, vp, u64, u64, u32, vp]
    lib.mv_index_insert_stored.argtypes = [vp, vp, u64, vp]
    lib.mv_connect_blocks.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp, u64, vp, vp, u64, vp]
    lib.mv_dev_connect_blocks.argtypes = [vp, ctypes.c_int, vp, u64, vp, vp, vp, u32, vp, vp, vp, u64, vp, vp, u64, vp, vp]
    lib.mv_pending_reserve.argtypes = [vp, u64, u64]
    lib.mv_pending_stats.argtypes = [vp, vp]
    lib.mv_dag_reserve.argtypes = [vp, u64, u64]
    lib.mv_dag_prune.argtypes = [vp, u64]
    lib.mv_dag_stats.argtypes = [vp, vp]
    lib.mv_decide_leaders.argtypes = [vp, vp, u32, vp, vp]
    lib.mv_dev_decide_leaders.argtypes = [vp, ctypes.c_int, vp, u32, vp, vp, vp]
    lib.mv_commit_leaders.argtypes = [vp, vp, u32, vp, vp, vp]
    lib.mv_dev_commit_leaders.argtypes = [vp, ctypes.c_int, vp, u32, vp, vp, vp, vp]
    lib.mv_linearize.argtypes = [vp, vp, u32, vp, u64, vp, vp]
    lib.mv_dev_linearize.argtypes = [vp, ctypes.c_int, vp, u32, vp, u64, vp, vp, vp]
    lib.mv_linearize_mark.argtypes = [vp, vp, u64, u64]
    lib.mv_linearize_stats.argtypes = [vp, vp]
    lib.mv_propose_reserve.argtypes = [vp, u32, u64]
    lib.mv_propose_add.argtypes = [vp, vp, u64, u64, vp, u32, u64, vp]
    lib.mv_dev_propose_add.argtypes = [vp, ctypes.c_int, vp, u64, u64, vp, u32, u64, vp, vp]
    lib.mv_propose_take.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp]
    lib.mv_propose_own.argtypes = [vp, vp, vp, u64, vp]
    lib.mv_propose_stats.argtypes = [vp, vp]
    lib.mv_host_alloc.argtypes = [vp, u64, ctypes.POINTER(vp)]
    lib.mv_host_free.argtypes = [vp, vp]
    lib.mv_host_free.restype = None
    lib.mv_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    lib.mv_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    for name in EXPORTS:
        getattr(lib, name).restype = getattr(lib, name).restype or ctypes.c_int32
    _lib = lib
    return lib


def _p(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _u8(a, shape_tail: int) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    return a.reshape(-1, shape_tail)


class Engine:
    """One mv_ctx: the devices it shards over, their streams and buffers."""

    def __init__(self, devices: Sequence[int] = (0,), max_batch: int = 0, batch: bool = True, comb: bool = True,
                 host_parse: bool = False, shards_per_device: int = 1, online: bool = True):
        """batch=False sets MV_FLAG_NO_BATCH: host-buffer verifies check every signature alone.
        comb=False sets MV_FLAG_NO_COMB: committee keys go through the per-signature ladder,
        not the per-key comb tables. host_parse=True sets MV_FLAG_HOST_PARSE: verify_blocks
        parses the bincode on the host instead of on the GPU. shards_per_device > 1 makes
        that many logical shards per device (host calls shard across them as across GPUs).
        online=False sets MV_FLAG_NO_ONLINE: small verify_blocks calls skip the resident online
        service and go through the submission queue."""
        self.lib = load_library()
        mask = 0
        for d in devices:
            mask |= 1 << int(d)
        flags = (0 if batch else FLAG_NO_BATCH) | (0 if comb else FLAG_NO_COMB) | (FLAG_HOST_PARSE if host_parse else 0) \
            | (0 if online else FLAG_NO_ONLINE)
        cfg = _Config(mask, max_batch, flags, shards_per_device)
        h = ctypes.c_void_p()
        rc = self.lib.mv_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != MV_OK:
            raise MvError(f"mv_create failed ({rc}): no usable gfx950 device")
        self.ctx = h
        self.devices = list(devices)
        self.committee_size = 0  # authorities of the committee in force (set_committee)

    def close(self):
        if getattr(self, "ctx", None):
            for ptr in getattr(self, "_pinned", {}).values():
                self.lib.mv_host_free(self.ctx, ptr)
            self._pinned = {}
            self.lib.mv_destroy(self.ctx)
            self.ctx = None

    def host_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array in page-locked host memory (mv_host_alloc), valid until close(): verify
        inputs held in such arrays are streamed to the GPU beside the verification."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = ctypes.c_void_p()
        self._check(self.lib.mv_host_alloc(self.ctx, max(nbytes, 1), ctypes.byref(ptr)), "mv_host_alloc")
        if not hasattr(self, "_pinned"):
            self._pinned = {}
        self._pinned[ptr.value] = ptr
        raw = (ctypes.c_uint8 * max(nbytes, 1)).from_address(ptr.value)
        return np.frombuffer(raw, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)

    def host_free(self, arr: np.ndarray):
        """Releases an array from host_empty (it must not be used afterwards)."""
        ptr = getattr(self, "_pinned", {}).pop(arr.__array_interface__["data"][0], None)
        if ptr is not None:
            self.lib.mv_host_free(self.ctx, ptr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != MV_OK:
            raise MvError(f"{what} failed ({rc}): {self.lib.mv_last_error(self.ctx).decode()}", rc)

    # ---- runtime switches (mv_set_option: the environment is read once, at mv_create) ----
    def set_option(self, name: str, value: int):
        self._check(self.lib.mv_set_option(self.ctx, name.encode(), int(value)), f"mv_set_option({name})")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        self._check(self.lib.mv_get_option(self.ctx, name.encode(), ctypes.byref(v)), f"mv_get_option({name})")
        return v.value

    @contextlib.contextmanager
    def option(self, name: str, value: int):
        """Sets a runtime switch for the duration of a with-block (then restores it)."""
        old = self.get_option(name)
        self.set_option(name, value)
        try:
            yield self
        finally:
            self.set_option(name, old)

    # ---- committee ----
    def set_committee(self, pks, stakes, epoch: int = 0) -> np.ndarray:
        pks = _u8(pks, 32)
        stakes = np.ascontiguousarray(np.asarray(stakes, dtype=np.uint64))
        ok = np.zeros(pks.shape[0], dtype=np.uint8)
        self._check(self.lib.mv_set_committee(self.ctx, _p(pks), _p(stakes), pks.shape[0], epoch, _p(ok)),
                    "mv_set_committee")
        self.committee_size = pks.shape[0]
        return ok

    # ---- hashes ----
    def blake2b256(self, items: Sequence[bytes]) -> List[bytes]:
        n = len(items)
        lens = np.array([len(x) for x in items], dtype=np.uint64)
        offs = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        buf = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)
        out = np.zeros((n, 32), dtype=np.uint8)
        self._check(self.lib.mv_blake2b256(self.ctx, _p(buf), _p(offs), _p(lens), n, _p(out)), "mv_blake2b256")
        return [bytes(r) for r in out]

    # ---- signatures ----
    def ed25519_verify(self, msg, sig, pk=None, key_idx=None) -> np.ndarray:
        msg, sig = _u8(msg, 32), _u8(sig, 64)
        n = msg.shape[0]
        pk_a = _u8(pk, 32) if pk is not None else None
        ki = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32)) if key_idx is not None else None
        st = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.mv_ed25519_verify(self.ctx, _p(msg), _p(sig), _p(pk_a), _p(ki), n, _p(st)),
                    "mv_ed25519_verify")
        return st

    def ed25519_sign(self, seed, msg) -> Tuple[np.ndarray, np.ndarray]:
        seed, msg = _u8(seed, 32), _u8(msg, 32)
        n = seed.shape[0]
        pk = np.zeros((n, 32), dtype=np.uint8)
        sig = np.zeros((n, 64), dtype=np.uint8)
        self._check(self.lib.mv_ed25519_sign(self.ctx, _p(seed), _p(msg), n, _p(pk), _p(sig)), "mv_ed25519_sign")
        return pk, sig

    # ---- blocks ----
    def verify_blocks(self, blocks: Sequence[bytes]):
        """StatementBlock::verify for each bincode Data<StatementBlock>: (status, msg_digest, block_digest)."""
        n = len(blocks)
        lens = np.array([len(b) for b in blocks], dtype=np.uint64)
        offs = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        buf = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
        return self.verify_blocks_packed(buf, offs, lens)

    def verify_blocks_packed(self, buf: np.ndarray, offs: np.ndarray, lens: np.ndarray):
        n = offs.shape[0]
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        md = np.zeros((n, 32), dtype=np.uint8)
        bd = np.zeros((n, 32), dtype=np.uint8)
        self._check(self.lib.mv_verify_blocks(self.ctx, _p(buf), _p(offs), _p(lens), n, _p(st), _p(md), _p(bd)),
                    "mv_verify_blocks")
        return st, md, bd

    def seal_blocks(self, buf: np.ndarray, offs, lens, seeds, link: bool = False):
        """StatementBlock::new_with_signer on bincode blocks whose digest and signature fields are
        placeholders (mv_seal_blocks): `buf` (a writable uint8 array) is patched in place with each
        block's signature under seeds[authority] and its digest; link=True also writes the fresh
        digests into the includes that name blocks of the call, round by round. Returns
        (status MV_SEAL_*, msg_digest, block_digest)."""
        if not (isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.flags.c_contiguous and
                buf.flags.writeable):
            raise ValueError("seal_blocks patches buf in place: a writable contiguous uint8 array")
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = offs.shape[0]
        if n and int((offs + lens).max()) > buf.shape[0]:
            raise ValueError("a block reaches past the buffer")
        seeds = _u8(seeds, 32)
        st = np.zeros(n, dtype=np.uint8)
        md = np.zeros((n, 32), dtype=np.uint8)
        bd = np.zeros((n, 32), dtype=np.uint8)
        self._check(self.lib.mv_seal_blocks(self.ctx, _p(buf), _p(offs), _p(lens), n, _p(seeds), seeds.shape[0],
                                            SEAL_LINK if link else 0, _p(st), _p(md), _p(bd)), "mv_seal_blocks")
        return st, md, bd

    def dev_seal_blocks(self, device: int, d_buf, buf_bytes: int, d_off, d_len, d_seeds, d_status, d_md=None,
                        d_bd=None, link: bool = False, stream_handle: int = 0):
        """mv_seal_blocks on HBM-resident bincode (torch uint8 buffer padded by 16 bytes, int64
        offsets and lengths, uint8 seeds [n_auth, 32]): the image is patched in place.
        Synchronises the stream."""
        vp = ctypes.c_void_p
        self._check(self.lib.mv_dev_seal_blocks(
            self.ctx, device, vp(d_buf.data_ptr()), int(buf_bytes), vp(d_off.data_ptr()), vp(d_len.data_ptr()),
            d_off.shape[0], vp(d_seeds.data_ptr()), d_seeds.shape[0], SEAL_LINK if link else 0,
            vp(d_status.data_ptr()), vp(d_md.data_ptr()) if d_md is not None else None,
            vp(d_bd.data_ptr()) if d_bd is not None else None, vp(stream_handle or None)), "mv_dev_seal_blocks")

    # ---- encoding blocks (core.rs:264-291, types.rs:93-114, data.rs:43-52) ----
    def encode_blocks(self, heads, includes, payloads, seal: bool = False, link: bool = False, seeds=None,
                      cap: Optional[int] = None, out: Optional[np.ndarray] = None) -> "EncodeResult":
        """The bincode of Core::try_new_block's blocks (mv_encode_blocks). heads: n x 10 words
        (authority, round, time low, time high, epoch, marker, first include row, include count,
        first payload, payload count); includes: m x 6 reference words, the own last block first in a
        block's run; payloads: a list of bincode::serialize(&Vec<BaseStatement>) strings (packed back
        to back here) or (buf, off, len) arrays. seal=True runs mv_seal_blocks' body on the image
        (seeds: n_auth x 32), link=True with MV_SEAL_LINK. cap: the room for the blocks (default: an
        upper bound from the heads and payload lengths); out: a uint8 array to write into (cap =
        its size). Returns EncodeResult; when out_bytes > cap nothing was written or sealed."""
        heads = np.ascontiguousarray(heads, dtype=np.uint64).reshape(-1, ENCODE_HEAD_WORDS)
        includes = np.ascontiguousarray(includes, dtype=np.uint64).reshape(-1, 6)
        if isinstance(payloads, tuple):
            pbuf, poff, plen = payloads
            pbuf = np.ascontiguousarray(pbuf, dtype=np.uint8)
            poff = np.ascontiguousarray(poff, dtype=np.uint64)
            plen = np.ascontiguousarray(plen, dtype=np.uint64)
        else:
            plen = np.array([len(x) for x in payloads], dtype=np.uint64)
            poff = np.zeros(len(payloads), dtype=np.uint64)
            if len(payloads) > 1:
                poff[1:] = np.cumsum(plen)[:-1]
            pbuf = np.frombuffer(b"".join(payloads), dtype=np.uint8)
        n, m, p = heads.shape[0], includes.shape[0], poff.shape[0]
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and
                    out.flags.writeable):
                raise ValueError("out: a writable contiguous uint8 array")
            cap = out.shape[0] if cap is None else int(cap)
            if cap > out.shape[0]:
                raise ValueError("cap reaches past out")
        else:
            if cap is None:
                cap = encode_bound(heads, m, plen)
            out = np.zeros(int(cap), dtype=np.uint8)
        if link and not seal:
            raise ValueError("link=True needs seal=True")
        flags = (ENCODE_SEAL if seal else 0) | (ENCODE_LINK if link else 0)
        seeds = _u8(seeds, 32) if seeds is not None else np.zeros((0, 32), dtype=np.uint8)
        offs = np.zeros(n, dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        total = ctypes.c_uint64(0)
        sst = np.zeros(n, dtype=np.uint8) if seal else None
        md = np.zeros((n, 32), dtype=np.uint8) if seal else None
        bd = np.zeros((n, 32), dtype=np.uint8) if seal else None
        self._check(self.lib.mv_encode_blocks(
            self.ctx, _p(heads), n, _p(includes) if m else None, m, _p(pbuf) if pbuf.shape[0] else None, pbuf.shape[0],
            _p(poff) if p else None, _p(plen) if p else None, p, flags, _p(seeds) if seeds.shape[0] else None,
            seeds.shape[0], _p(out) if cap else None, int(cap), _p(offs), _p(lens), _p(st), ctypes.byref(total), _p(sst),
            _p(md), _p(bd)), "mv_encode_blocks")
        return EncodeResult(out, offs, lens, st, int(total.value), sst, md, bd)

    def dev_encode_blocks(self, device: int, d_heads, d_includes, d_payload_buf, payload_bytes: int, d_payload_off,
                          d_payload_len, d_out, cap: int, d_out_off, d_out_len, d_status, seal: bool = False,
                          link: bool = False, d_seeds=None, d_seal_status=None, d_md=None, d_bd=None,
                          stream_handle: int = 0) -> int:
        """mv_encode_blocks on HBM-resident arrays (torch tensors: int64 heads [n, 10], includes [m, 6],
        payload offsets and lengths; uint8 payload bytes padded by 16 bytes past payload_bytes and an
        image padded by 16 bytes past cap). Returns *out_bytes. Synchronises the stream for the total."""
        vp = ctypes.c_void_p

        def ptr(t):
            return vp(t.data_ptr()) if t is not None and t.numel() else None

        flags = (ENCODE_SEAL if seal else 0) | (ENCODE_LINK if link else 0)
        total = ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_encode_blocks(
            self.ctx, device, ptr(d_heads), d_heads.shape[0], ptr(d_includes), d_includes.shape[0], ptr(d_payload_buf),
            int(payload_bytes), ptr(d_payload_off), ptr(d_payload_len), d_payload_off.shape[0], flags, ptr(d_seeds),
            d_seeds.shape[0] if d_seeds is not None else 0, ptr(d_out), int(cap), ptr(d_out_off), ptr(d_out_len),
            ptr(d_status), ctypes.byref(total), ptr(d_seal_status), ptr(d_md), ptr(d_bd), vp(stream_handle or None)),
            "mv_dev_encode_blocks")
        return int(total.value)

    # ---- transaction votes (committee.rs:263-482) ----
    def votes_reserve(self, blocks: int, cells: int):
        """Makes the vote store, or grows it, for `blocks` sharing blocks and `cells` statement offsets
        (mv_votes_reserve; needs set_committee)."""
        self._check(self.lib.mv_votes_reserve(self.ctx, int(blocks), int(cells)), "mv_votes_reserve")

    def votes_clear(self):
        self._check(self.lib.mv_votes_clear(self.ctx), "mv_votes_clear")

    def votes_stats(self) -> "VotesStats":
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_votes_stats(self.ctx, _p(out)), "mv_votes_stats")
        return VotesStats(*(int(x) for x in out))

    def aggregate_votes(self, blocks: Sequence[bytes], register_only: bool = False, cap_certified: Optional[int] = None):
        """TransactionAggregator::process_block for each bincode block, in order (mv_aggregate_votes).
        Returns (status MV_VOTES_*, counts (n, 4) uint64: certified, unknown, duplicate, flag bits,
        certified rows (k, 8) uint64: reference words 0-5, offset, certifying block, total certified);
        k = min(total, cap_certified), by default all of them."""
        n = len(blocks)
        lens = np.array([len(b) for b in blocks], dtype=np.uint64)
        offs = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        buf = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        counts = np.zeros((max(n, 1), 4), dtype=np.uint64)
        total = ctypes.c_uint64(0)
        flags = VOTES_REGISTER_ONLY if register_only else 0
        cap = 1024 if cap_certified is None else int(cap_certified)
        rows = np.zeros((max(cap, 1), 8), dtype=np.uint64)
        self._check(self.lib.mv_aggregate_votes(self.ctx, _p(buf), _p(offs), _p(lens), n, flags, _p(st), _p(counts),
                                                _p(rows), cap, ctypes.byref(total)), "mv_aggregate_votes")
        if cap_certified is None and total.value > cap:
            raise MvError("aggregate_votes: more than 1024 transactions certified; pass cap_certified (the store has "
                          "advanced)")
        return st[:n], counts[:n], rows[:min(total.value, cap)].copy(), int(total.value)

    def dev_aggregate_votes(self, device: int, d_buf, buf_bytes: int, d_off, d_len, d_status, d_counts, d_certified=None,
                            register_only: bool = False, stream_handle: int = 0) -> int:
        """mv_aggregate_votes on HBM-resident bincode (torch uint8 buffer padded by 16 bytes, int64
        offsets and lengths, uint8 status, int64 counts (n, 4) and certified rows (cap, 8)).
        Synchronises the stream; returns the certified total."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64(0)
        cap = d_certified.shape[0] if d_certified is not None else 0
        self._check(self.lib.mv_dev_aggregate_votes(
            self.ctx, device, vp(d_buf.data_ptr()), int(buf_bytes), vp(d_off.data_ptr()), vp(d_len.data_ptr()),
            d_off.shape[0], VOTES_REGISTER_ONLY if register_only else 0, vp(d_status.data_ptr()),
            vp(d_counts.data_ptr()), vp(d_certified.data_ptr()) if cap else None, cap, ctypes.byref(total),
            vp(stream_handle or None)), "mv_dev_aggregate_votes")
        return int(total.value)

    def verify_frames(self, buf):
        """Blocks of received NetworkMessage frames (network.rs:400-447) verified in place:
        mv_frame_blocks lists them, mv_verify_blocks checks them on the same buffer. Returns
        (status, msg_digest, block_digest, consumed bytes of complete frames)."""
        buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf,
                                   dtype=np.uint8)
        offs, lens, consumed = frame_blocks(buf)
        st, md, bd = self.verify_blocks_packed(buf, offs, lens)
        return st, md, bd, consumed

    def verify_frames_messages(self, buf, soff, slen) -> "FrameVerdicts":
        """The received bytes of many connections verified per message (mv_verify_frames:
        handle_read_stream, the NetworkMessage decode and process_blocks, network.rs:400-457,
        net_sync.rs:314-383). Stream s is buf[soff[s], soff[s] + slen[s]). Returns a FrameVerdicts:
        one row per message (n x 8 uint32), consumed bytes and the first dropped row per stream,
        and the listed blocks with their MV_BLOCK_* statuses."""
        buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf,
                                   dtype=np.uint8)
        soff = np.ascontiguousarray(np.asarray(soff, dtype=np.uint64))
        slen = np.ascontiguousarray(np.asarray(slen, dtype=np.uint64))
        ns = soff.shape[0]
        if ns and int((soff + slen).max()) > buf.size:
            raise ValueError("a stream reaches past the buffer")
        consumed = np.zeros(max(ns, 1), dtype=np.uint64)
        drop = np.zeros(max(ns, 1), dtype=np.uint32)
        nm, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        pb = _p(buf) if buf.size else _p(np.zeros(1, dtype=np.uint8))
        # a frame takes at least 5 bytes and a block at least its 8-byte length; large inputs start
        # from a guess below that bound, and a call whose totals exceed it is repeated at the totals
        total = int(slen.sum()) if ns else 0
        cap_m = min(total // 5 + 1, max(1 << 16, total // 256))
        cap_b = min(total // 8 + 1, max(1 << 16, total // 128))
        while True:
            rows = np.zeros((cap_m, 8), dtype=np.uint32)
            off = np.zeros(cap_b, dtype=np.uint64)
            ln = np.zeros(cap_b, dtype=np.uint64)
            st = np.zeros(cap_b, dtype=np.uint8)
            self._check(self.lib.mv_verify_frames(self.ctx, pb, _p(soff), _p(slen), ns, _p(consumed), _p(drop),
                                                  _p(rows), cap_m, ctypes.byref(nm), _p(off), _p(ln), _p(st), cap_b,
                                                  ctypes.byref(nb)), "mv_verify_frames")
            n, b = int(nm.value), int(nb.value)
            if n <= cap_m and b <= cap_b:
                break
            cap_m, cap_b = max(cap_m, n), max(cap_b, b)
        return FrameVerdicts(rows[:n].copy(), consumed[:ns].copy(), drop[:ns].copy(), off[:b].copy(), ln[:b].copy(),
                             st[:b].copy())

    # ---- device-resident (torch tensors on the device) ----
    def dev_verify_frames(self, device: int, d_buf, buf_bytes: int, d_soff, d_slen, d_consumed, d_drop_msg, d_msgs,
                          d_blk_off, d_blk_len, d_blk_status=None, stream_handle: int = 0) -> Tuple[int, int]:
        """mv_dev_verify_frames on torch device tensors (d_buf uint8, 8-byte aligned with 16 readable
        bytes past buf_bytes; d_soff / d_slen / d_consumed / d_blk_off / d_blk_len int64; d_drop_msg
        and d_msgs (cap x 8) int32; d_blk_status uint8). Synchronises the stream; returns the
        (message, block) totals, of which the first d_msgs.shape[0] / d_blk_off.shape[0] are written."""
        vp = ctypes.c_void_p
        nm, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_verify_frames(
            self.ctx, device, vp(d_buf.data_ptr()), int(buf_bytes), vp(d_soff.data_ptr()), vp(d_slen.data_ptr()),
            d_soff.shape[0], vp(d_consumed.data_ptr()), vp(d_drop_msg.data_ptr()), vp(d_msgs.data_ptr()),
            d_msgs.shape[0], ctypes.byref(nm), vp(d_blk_off.data_ptr()), vp(d_blk_len.data_ptr()),
            vp(d_blk_status.data_ptr()) if d_blk_status is not None else None, d_blk_off.shape[0], ctypes.byref(nb),
            vp(stream_handle or None)), "mv_dev_verify_frames")
        return int(nm.value), int(nb.value)

    def dev_verify(self, device: int, d_msg, d_sig, d_pk, d_status, stream_handle: int = 0):
        n = d_msg.shape[0]
        self._check(self.lib.mv_dev_ed25519_verify(self.ctx, device, ctypes.c_void_p(d_msg.data_ptr()),
                                                   ctypes.c_void_p(d_sig.data_ptr()), ctypes.c_void_p(d_pk.data_ptr()),
                                                   n, ctypes.c_void_p(d_status.data_ptr()),
                                                   ctypes.c_void_p(stream_handle or None)),
                    "mv_dev_ed25519_verify")

    def dev_verify_batch(self, device: int, d_msg, d_sig, d_pk, d_status, d_batch_ok=None, stream_handle: int = 0,
                         d_key_idx=None):
        """Batch path (one combined equation, exact fallback) on device tensors; enqueue only."""
        n = d_msg.shape[0]
        vp = ctypes.c_void_p
        self._check(self.lib.mv_dev_ed25519_verify_batch(
            self.ctx, device, vp(d_msg.data_ptr()), vp(d_sig.data_ptr()), vp(d_pk.data_ptr()),
            vp(d_key_idx.data_ptr()) if d_key_idx is not None else None, n, vp(d_status.data_ptr()),
            vp(d_batch_ok.data_ptr()) if d_batch_ok is not None else None, vp(stream_handle or None)),
            "mv_dev_ed25519_verify_batch")

    def batch_stats(self) -> Tuple[int, int]:
        """(batches tried, batches that fell back to per-signature verification) on the host path."""
        b, f = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.mv_batch_stats(self.ctx, ctypes.byref(b), ctypes.byref(f)), "mv_batch_stats")
        return b.value, f.value

    def batch_counters(self) -> Tuple[int, int, int, int]:
        """(batches, batches with a failed equation, sub-batch equations, failed sub-batch equations)."""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_batch_counters(self.ctx, _p(out)), "mv_batch_counters")
        return tuple(int(x) for x in out)

    def batch_routes(self) -> Tuple[int, int, int]:
        """(batches checked by a combined equation, batches verified signature by signature
        because failures were dense, dense failures seen)."""
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.mv_batch_routes(self.ctx, _p(out)), "mv_batch_routes")
        return tuple(int(x) for x in out)

    def set_batch_groups(self, groups: int):
        """Sub-batch equations per batch: 0 = adaptive (default), 1..16 fixed."""
        self._check(self.lib.mv_set_batch_groups(self.ctx, int(groups)), "mv_set_batch_groups")

    def queue_stats(self) -> Tuple[int, int]:
        """(mv_verify_blocks calls, device passes that served them)."""
        c, p = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.mv_queue_stats(self.ctx, ctypes.byref(c), ctypes.byref(p)), "mv_queue_stats")
        return c.value, p.value

    def online_stats(self) -> Tuple[int, int]:
        """(verify_blocks calls served by the resident online service, its kernel launches)."""
        r, l = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.mv_online_stats(self.ctx, ctypes.byref(r), ctypes.byref(l)), "mv_online_stats")
        return r.value, l.value

    def set_stage_timing(self, enable: bool = True):
        self._check(self.lib.mv_set_stage_timing(self.ctx, 1 if enable else 0), "mv_set_stage_timing")

    def stage_times(self, reset: bool = False):
        """({stage: summed device ms}, {stage: calls measured}) since the last reset."""
        ms = np.zeros(len(STAGES), dtype=np.float64)
        calls = np.zeros(len(STAGES), dtype=np.uint64)
        self._check(self.lib.mv_stage_times(self.ctx, _p(ms), _p(calls), 1 if reset else 0), "mv_stage_times")
        return dict(zip(STAGES, ms.tolist())), dict(zip(STAGES, (int(c) for c in calls)))

    def dev_verify_blocks(self, device: int, d_buf, buf_bytes: int, d_off, d_len, d_status, d_md=None, d_bd=None,
                          stream_handle: int = 0):
        """StatementBlock::verify on HBM-resident bincode (torch uint8 buffer, int64 offsets and
        lengths); parse, digests, signatures and checks on the GPU. Enqueue only."""
        n = d_off.shape[0]
        vp = ctypes.c_void_p
        self._check(self.lib.mv_dev_verify_blocks(
            self.ctx, device, vp(d_buf.data_ptr()), int(buf_bytes), vp(d_off.data_ptr()), vp(d_len.data_ptr()), n,
            vp(d_status.data_ptr()), vp(d_md.data_ptr()) if d_md is not None else None,
            vp(d_bd.data_ptr()) if d_bd is not None else None, vp(stream_handle or None)), "mv_dev_verify_blocks")

    def dev_sign(self, device: int, d_seed, d_msg, d_pk, d_sig, stream_handle: int = 0):
        n = d_seed.shape[0]
        self._check(self.lib.mv_dev_ed25519_sign(self.ctx, device, ctypes.c_void_p(d_seed.data_ptr()),
                                                 ctypes.c_void_p(d_msg.data_ptr()), n,
                                                 ctypes.c_void_p(d_pk.data_ptr()), ctypes.c_void_p(d_sig.data_ptr()),
                                                 ctypes.c_void_p(stream_handle or None)),
                    "mv_dev_ed25519_sign")

    # ---- WAL replay (wal.rs) ----
    def crc32(self, items: Sequence[bytes]) -> np.ndarray:
        """crc32fast::hash of every item (uint32 array)."""
        items = [bytes(x) for x in items]
        lens = np.array([len(x) for x in items], dtype=np.uint64)
        offs = np.zeros(len(items), dtype=np.uint64)
        if len(items) > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        buf = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)
        return self.crc32_packed(buf, offs, lens)

    def crc32_packed(self, buf: np.ndarray, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offs)
        out = np.zeros(n, dtype=np.uint32)
        if n:
            self._check(self.lib.mv_crc32(self.ctx, _p(buf), _p(offs), _p(lens), n, _p(out)), "mv_crc32")
        return out

    def wal_verify(self, image, end_pos: Optional[int] = None, map_bits: int = WAL_MAP_BITS,
                   cap: Optional[int] = None):
        """WalReader::iter_until over a WAL image (bytes / uint8 array) up to the writer position
        end_pos (default: its length). Returns (pos, tag, len, status) arrays of the entries in
        iteration order, the last one failing (status != WAL_OK) where the reference panics."""
        img = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                                   else np.asarray(image, dtype=np.uint8))
        size = img.size
        end = size if end_pos is None else int(end_pos)
        if cap is None:
            cap = size // 16 + 1
        pos = np.zeros(max(cap, 1), dtype=np.uint64)
        tag = np.zeros(max(cap, 1), dtype=np.uint32)
        ln = np.zeros(max(cap, 1), dtype=np.uint32)
        st = np.zeros(max(cap, 1), dtype=np.uint8)
        cnt = ctypes.c_uint64(0)
        self._check(self.lib.mv_wal_verify(self.ctx, _p(img) if size else None, size, end, map_bits, _p(pos),
                                           _p(tag), _p(ln), _p(st), cap, ctypes.byref(cnt)), "mv_wal_verify")
        n = min(cnt.value, cap)
        return pos[:n], tag[:n], ln[:n], st[:n]

    def wal_iter_until(self, image, end_pos: Optional[int] = None, map_bits: int = WAL_MAP_BITS):
        """The reference's iterator (wal.rs:270-346): yields (position, (tag, payload bytes)) and
        raises MvError with the reference's panic message where it would panic."""
        img = bytes(image)
        pos, tag, ln, st = self.wal_verify(img, end_pos, map_bits)
        for p, t, n, s in zip(pos.tolist(), tag.tolist(), ln.tolist(), st.tolist()):
            if s == WAL_CRC_MISMATCH:
                hdr = int.from_bytes(img[p:p + 16].ljust(16, b"\0"), "little")
                full = (hdr >> 64) & 0xFFFFFFFF
                found = int(self.crc32([img[p + 16:p + full].ljust(full - 16, b"\0")])[0])
                raise MvError(f"Crc mismatch, expected {hdr & ((1 << 64) - 1)}, found {found} at position {p}:{full}")
            if s == WAL_NONZERO_CRC_LEN0:
                crc = int.from_bytes(img[p:p + 8].ljust(8, b"\0"), "little")
                raise MvError(f"Non-zero crc at len 0, crc: {crc}, position:{p}")
            if s == WAL_BAD_LENGTH:
                raise MvError(f"entry at position {p} runs outside its map (Bytes::slice out of range)")
            yield p, (t, img[p + 16:p + 16 + n])

    def dev_wal_verify(self, device: int, d_img, size: int, end_pos: int, map_bits: int, d_pos, d_tag, d_len,
                       d_status, cap: int, stream_handle: int = 0) -> int:
        """mv_dev_wal_verify on torch device tensors; returns the entry count."""
        cnt = ctypes.c_uint64(0)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.mv_dev_wal_verify(self.ctx, device, ptr(d_img), size, end_pos, map_bits, ptr(d_pos),
                                               ptr(d_tag), ptr(d_len), ptr(d_status), cap, ctypes.byref(cnt),
                                               ctypes.c_void_p(stream_handle or None)), "mv_dev_wal_verify")
        return cnt.value

    def wal_replay(self, image, end_pos: Optional[int] = None, map_bits: int = WAL_MAP_BITS,
                   cap: Optional[int] = None, cap_blocks: Optional[int] = None, _recover_floor: Optional[int] = None):
        """The replay loop of BlockStore::open (mv_wal_replay, block_store.rs:50-116) over a WAL image
        (bytes / uint8 array) up to the writer position end_pos (default: its length). Needs
        set_committee. Returns a WalReplay: the entries as wal_verify gives them (the last one
        failing where the reference panics: also an unknown tag, a block that does not decode, an
        authority outside the committee), one row per decoded block with its StatementBlock::verify
        status, the summary words and last_seen_by_authority. cap / cap_blocks below the totals:
        only that many entries / rows are returned (count and n_blocks are always the totals)."""
        img = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                                   else np.asarray(image, dtype=np.uint8))
        size = img.size
        end = size if end_pos is None else int(end_pos)
        if cap is None:
            cap = size // 16 + 1
        if cap_blocks is None:
            cap_blocks = size // 72 + 1  # a block entry: header 16 + its own reference 56 at least
        n_auth = self.committee_size
        pos = np.zeros(max(cap, 1), dtype=np.uint64)
        tag = np.zeros(max(cap, 1), dtype=np.uint32)
        ln = np.zeros(max(cap, 1), dtype=np.uint32)
        st = np.zeros(max(cap, 1), dtype=np.uint8)
        rows = np.zeros((max(cap_blocks, 1), WAL_ROW_WORDS), dtype=np.uint64)
        bst = np.zeros(max(cap_blocks, 1), dtype=np.uint8)
        summary = np.zeros(3, dtype=np.uint64)
        seen = np.zeros(max(n_auth, 1), dtype=np.uint64)
        cnt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        args = (self.ctx, _p(img) if size else None, size, end, map_bits, _p(pos), _p(tag), _p(ln), _p(st), cap,
                ctypes.byref(cnt), _p(rows), _p(bst), cap_blocks, ctypes.byref(nb), _p(summary), _p(seen))
        seeded = np.zeros(5, dtype=np.uint64)
        if _recover_floor is None:
            self._check(self.lib.mv_wal_replay(*args), "mv_wal_replay")
        else:
            self._check(self.lib.mv_wal_recover(*args, int(_recover_floor), _p(seeded)), "mv_wal_recover")
        n, b = min(cnt.value, cap), min(nb.value, cap_blocks)
        out = WalReplay(pos[:n], tag[:n], ln[:n], st[:n], rows[:b], bst[:b], summary, seen[:n_auth], cnt.value, nb.value)
        return out if _recover_floor is None else (out, Seeded(*(int(x) for x in seeded)))

    def wal_recover(self, image, end_pos: Optional[int] = None, map_bits: int = WAL_MAP_BITS, floor_round: int = 0,
                    cap: Optional[int] = None, cap_blocks: Optional[int] = None) -> Tuple["WalReplay", "Seeded"]:
        """wal_replay, then the replayed blocks become stored blocks with records in the DAG store
        (mv_wal_recover: BlockStore::open with add_unloaded, block_store.rs:398-404). Needs set_committee
        and dag_reserve. floor_round: rows of lower rounds get no record, as after dag_prune. Returns
        the WalReplay that wal_replay returns and a Seeded."""
        return self.wal_replay(image, end_pos, map_bits, cap, cap_blocks, _recover_floor=int(floor_round))

    def dev_dag_seed_rows(self, device: int, d_img, size: int, d_rows, d_blk_status, n_rows: Optional[int] = None,
                          floor_round: int = 0, stream_handle: int = 0, img_ptr: Optional[int] = None) -> "Seeded":
        """mv_dev_dag_seed_rows on torch device tensors: the image, rows ((n, 10) int64) and block
        verdicts (uint8) of a dev_wal_replay. Synchronises the stream. Raises MvError with code
        E_INDEX_FULL when the reserved index or the reserved DAG store has no room (both are unchanged).
        img_ptr overrides d_img's address."""
        vp = ctypes.c_void_p
        n = d_rows.shape[0] if n_rows is None else int(n_rows)
        seeded = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.mv_dev_dag_seed_rows(
            self.ctx, device, vp(img_ptr) if img_ptr is not None else vp(d_img.data_ptr()), int(size), vp(d_rows.data_ptr()),
            vp(d_blk_status.data_ptr()), n, int(floor_round), _p(seeded), vp(stream_handle or None)), "mv_dev_dag_seed_rows")
        return Seeded(*(int(x) for x in seeded))

    def dev_wal_replay(self, device: int, d_img, size: int, end_pos: int, map_bits: int, d_pos, d_tag, d_len,
                       d_status, d_rows, d_blk_status, d_summary, d_last_seen, stream_handle: int = 0,
                       img_ptr: Optional[int] = None) -> Tuple[int, int]:
        """mv_dev_wal_replay on torch device tensors (d_img uint8, 8-byte aligned with 16 readable
        bytes past size; d_pos int64, d_tag / d_len int32, d_status uint8 of cap entries; d_rows
        (cap_blocks x 10) int64; d_blk_status uint8 or None; d_summary (3) and d_last_seen (committee
        size) int64). Synchronises the stream; returns the (entry, row) totals, of which the first
        d_pos.shape[0] / d_rows.shape[0] are written. img_ptr overrides d_img's address."""
        cnt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.mv_dev_wal_replay(
            self.ctx, device, ctypes.c_void_p(img_ptr) if img_ptr is not None else ptr(d_img), size, end_pos, map_bits,
            ptr(d_pos), ptr(d_tag), ptr(d_len), ptr(d_status), d_pos.shape[0], ctypes.byref(cnt), ptr(d_rows),
            ptr(d_blk_status) if d_blk_status is not None else None, d_rows.shape[0], ctypes.byref(nb), ptr(d_summary),
            ptr(d_last_seen), ctypes.c_void_p(stream_handle or None)), "mv_dev_wal_replay")
        return cnt.value, nb.value

    # ---- the WAL write (wal.rs:150-188, block_store.rs:504-518, 542-549) ----
    def wal_write(self, entries, start: int = 0, map_bits: int = WAL_MAP_BITS, cap: Optional[int] = None,
                  out: Optional[np.ndarray] = None) -> "WalWrite":
        """The bytes WalWriter::writev appends for these entries to a file of length `start`
        (mv_wal_write). entries: (tag, bytes), or (3, next_entry, bytes) for an own block; or a
        tuple (buf, rows) of the payload bytes and (n, 4) uint64 rows tag | offset | length |
        next_entry. cap: the room for the bytes (default: what the entries need, from wal_layout);
        out: a uint8 array to write into (cap = its size). Returns a WalWrite; when end_pos - start
        exceeds cap its image is empty and nothing was written. Raises MvError with code
        E_INVALID_ARG for a body no map holds and for a payload outside buf."""
        if isinstance(entries, tuple):
            buf = np.ascontiguousarray(entries[0], dtype=np.uint8)
            rows = np.ascontiguousarray(entries[1], dtype=np.uint64).reshape(-1, 4)
        else:
            parts, rows, off = [], np.zeros((len(entries), 4), dtype=np.uint64), 0
            for i, e in enumerate(entries):
                tag, nxt, data = (e[0], 0, e[1]) if len(e) == 2 else e
                rows[i] = (tag, off, len(data), nxt)
                parts.append(bytes(data))
                off += len(data)
            buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
        n = rows.shape[0]
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and
                    out.flags.writeable):
                raise ValueError("out: a writable contiguous uint8 array")
            cap = out.shape[0] if cap is None else int(cap)
            if cap > out.shape[0]:
                raise ValueError("cap reaches past out")
        else:
            if cap is None:
                body = rows[:, 2] + np.where((rows[:, 0] & np.uint64(0xFFFFFFFF)) == 3, 8, 0).astype(np.uint64)
                cap = wal_layout(body, map_bits, int(start))[1] - int(start)
            out = np.zeros(int(cap), dtype=np.uint8)
        pos = np.zeros(max(n, 1), dtype=np.uint64)
        end = ctypes.c_uint64(0)
        self._check(self.lib.mv_wal_write(self.ctx, _p(buf) if buf.shape[0] else None, buf.shape[0],
                                          _p(rows) if n else None, n, int(start), map_bits, _p(out) if cap else None,
                                          int(cap), _p(pos), ctypes.byref(end)), "mv_wal_write")
        span = end.value - int(start)
        return WalWrite(out[:span] if span <= cap else out[:0], pos[:n], end.value)

    def dev_wal_write(self, device: int, d_buf, buf_bytes: int, d_entries, start: int, map_bits: int, d_out, cap: int,
                      d_pos, stream_handle: int = 0) -> int:
        """mv_dev_wal_write on torch device tensors (d_buf uint8, 8-byte aligned with 16 readable
        bytes past buf_bytes -- the buffer of a dev_encode_blocks, dev_seal_blocks or
        dev_connect_blocks call as it is; d_entries (n, 4) int64 rows; d_out uint8 of at least cap
        bytes; d_pos int64 of n). Synchronises the stream once; returns end_pos. When end_pos - start
        exceeds cap only d_pos was written."""
        vp = ctypes.c_void_p

        def ptr(t):
            return vp(t.data_ptr()) if t is not None and t.numel() else None

        end = ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_wal_write(self.ctx, device, ptr(d_buf), int(buf_bytes), ptr(d_entries),
                                              d_entries.shape[0], int(start), map_bits, ptr(d_out), int(cap), ptr(d_pos),
                                              ctypes.byref(end), vp(stream_handle or None)), "mv_dev_wal_write")
        return end.value

    def dev_crc32(self, device: int, d_buf, d_off, d_len, n: int, d_out, stream_handle: int = 0):
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.mv_dev_crc32(self.ctx, device, ptr(d_buf), ptr(d_off), ptr(d_len), n, ptr(d_out),
                                          ctypes.c_void_p(stream_handle or None)), "mv_dev_crc32")

    # ---- the index of block references (block_manager.rs) ----
    def index_reserve(self, entries: int):
        """Makes the index, or grows it so that `entries` references fit at a load of at most 1/2."""
        self._check(self.lib.mv_index_reserve(self.ctx, int(entries)), "mv_index_reserve")

    def index_clear(self):
        self._check(self.lib.mv_index_clear(self.ctx), "mv_index_clear")
        self._suspended = 0

    def index_stats(self) -> "IndexStats":
        out = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.mv_index_stats(self.ctx, _p(out)), "mv_index_stats")
        return IndexStats(*(int(x) for x in out))

    def index_insert(self, refs, state: int = REF_HAVE) -> np.ndarray:
        """Raises references ((n, 6) uint64 words, or (authority, round, digest) tuples) to `state`;
        returns the state each had before the call."""
        r = ref_words(refs)
        prior = np.zeros(r.shape[0], dtype=np.uint8)
        self._check(self.lib.mv_index_insert(self.ctx, _p(r), r.shape[0], int(state), _p(prior)), "mv_index_insert")
        return prior

    def index_insert_stored(self, refs) -> np.ndarray:
        """Raises references to REF_STORED (mv_index_insert_stored): blocks that are in the store --
        genesis, a replayed WAL, an own proposal. Returns the state each had before the call."""
        r = ref_words(refs)
        prior = np.zeros(r.shape[0], dtype=np.uint8)
        self._check(self.lib.mv_index_insert_stored(self.ctx, _p(r), r.shape[0], _p(prior)), "mv_index_insert_stored")
        return prior

    def index_lookup(self, refs) -> np.ndarray:
        """REF_* of every reference: REF_HAVE or REF_STORED is BlockManager::exists_or_pending,
        REF_STORED BlockStore::block_exists."""
        r = ref_words(refs)
        st = np.zeros(r.shape[0], dtype=np.uint8)
        self._check(self.lib.mv_index_lookup(self.ctx, _p(r), r.shape[0], _p(st)), "mv_index_lookup")
        return st

    def index_wanted(self, cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
        """The REF_WANTED references (BlockManager::missing_blocks) as (k, 6) uint64 words in no
        particular order, and their total (k = min(total, cap))."""
        n = ctypes.c_uint64(0)
        if cap is None:
            self._check(self.lib.mv_index_wanted(self.ctx, None, 0, ctypes.byref(n)), "mv_index_wanted")
            cap = int(n.value)
        out = np.zeros((max(cap, 1), 6), dtype=np.uint64)
        self._check(self.lib.mv_index_wanted(self.ctx, _p(out), cap, ctypes.byref(n)), "mv_index_wanted")
        return out[:min(int(n.value), cap)], int(n.value)

    def accept_blocks(self, blocks: Sequence[bytes], groups=None, cap_missing: Optional[int] = None) -> "Accepted":
        """One accept call (mv_accept_blocks) over bincode blocks; groups: one non-decreasing word
        per block naming its message, or None (every block a message of its own)."""
        buf, offs, lens = _pack(blocks)
        return self.accept_blocks_packed(buf, offs, lens, groups, cap_missing)

    def accept_blocks_packed(self, buf: np.ndarray, offs, lens, groups=None, cap_missing: Optional[int] = None,
                             missing_out: Optional[np.ndarray] = None) -> "Accepted":
        """mv_accept_blocks on blocks buf[offs[i], offs[i] + lens[i]). cap_missing None: room for every
        include (no list is cut). missing_out: the (cap, 6) uint64 array the call writes into."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = offs.shape[0]
        grp = None if groups is None else np.ascontiguousarray(np.asarray(groups, dtype=np.uint64))
        if grp is not None and grp.shape != (n,):
            raise ValueError("groups: one word per block")
        if cap_missing is None:
            cap_missing = int(lens.sum()) // 56 + 1  # an include takes 56 bytes
        miss = missing_out if missing_out is not None else np.zeros((max(cap_missing, 1), 6), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        state = np.zeros(max(n, 1), dtype=np.uint8)
        nm = ctypes.c_uint64(0)
        self._check(self.lib.mv_accept_blocks(self.ctx, _p(buf) if buf.size else None, _p(offs), _p(lens), _p(grp), n,
                                              _p(st), _p(state), _p(miss), cap_missing, ctypes.byref(nm)),
                    "mv_accept_blocks")
        return Accepted(st[:n], state[:n], miss[:min(int(nm.value), cap_missing)], int(nm.value))

    def dev_accept_blocks(self, device: int, d_buf, buf_bytes: int, d_off, d_len, d_grp, d_blk_status, d_blk_state,
                          d_missing, stream_handle: int = 0) -> int:
        """mv_dev_accept_blocks on torch device tensors (d_buf uint8, 8-byte aligned with 16 readable
        bytes past every block; d_off / d_len / d_grp int64, d_grp may be None; d_blk_status /
        d_blk_state uint8; d_missing (cap, 6) int64 or None). Synchronises the stream; returns the
        missing total, of which the first d_missing.shape[0] rows are written. Raises MvError with
        code E_INDEX_FULL when the reserved index has no room (the index is unchanged)."""
        vp = ctypes.c_void_p
        nm = ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_accept_blocks(
            self.ctx, device, vp(d_buf.data_ptr()), int(buf_bytes), vp(d_off.data_ptr()), vp(d_len.data_ptr()),
            vp(d_grp.data_ptr()) if d_grp is not None else None, d_off.shape[0], vp(d_blk_status.data_ptr()),
            vp(d_blk_state.data_ptr()), vp(d_missing.data_ptr()) if d_missing is not None else None,
            d_missing.shape[0] if d_missing is not None else 0, ctypes.byref(nm), vp(stream_handle or None)),
            "mv_dev_accept_blocks")
        return int(nm.value)

    def connect_blocks(self, blocks: Sequence[bytes] = (), groups=None, cap_missing: Optional[int] = None,
                       cap_connected: Optional[int] = None, connected_out: Optional[np.ndarray] = None) -> "Connected":
        """One connect call (mv_connect_blocks): accept_blocks, then every NEW block joins the
        suspended-block store and the store is swept. No blocks: a sweep alone. cap_connected None:
        room for every suspended block. connected_out: the (cap, 8) uint64 array the call writes into."""
        buf, offs, lens = _pack(list(blocks))
        n = offs.shape[0]
        grp = None if groups is None else np.ascontiguousarray(np.asarray(groups, dtype=np.uint64))
        if grp is not None and grp.shape != (n,):
            raise ValueError("groups: one word per block")
        if cap_missing is None:
            cap_missing = int(lens.sum()) // 56 + 1
        if cap_connected is None:
            # the suspended blocks as the host-buffer calls left them (an upper bound: no device
            # round trip to size a buffer); after a device-buffer call the library is asked
            known = getattr(self, "_suspended", None)
            cap_connected = n + (self.pending_stats().suspended if known is None else known)
        miss = np.zeros((max(cap_missing, 1), 6), dtype=np.uint64)
        rows = connected_out if connected_out is not None else np.zeros((max(cap_connected, 1), 8), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        state = np.zeros(max(n, 1), dtype=np.uint8)
        nm, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.mv_connect_blocks(self.ctx, _p(buf), _p(offs), _p(lens), _p(grp), n, _p(st), _p(state),
                                               _p(miss), cap_missing, ctypes.byref(nm), _p(rows), cap_connected,
                                               ctypes.byref(nc)), "mv_connect_blocks")
        if getattr(self, "_suspended", None) is not None:  # every NEW block joined the store, every row left it
            joined = int(np.isin(state[:n], (ACC_NEW, ACC_SUSPENDED)).sum())
            self._suspended = max(self._suspended + joined - int(nc.value), 0)
        return Connected(st[:n], state[:n], miss[:min(int(nm.value), cap_missing)], int(nm.value),
                         rows[:min(int(nc.value), cap_connected)], int(nc.value))

    def dev_connect_blocks(self, device: int, d_buf, buf_bytes: int, d_off, d_len, d_grp, d_blk_status, d_blk_state,
                           d_missing, d_connected, stream_handle: int = 0) -> Tuple[int, int]:
        """mv_dev_connect_blocks on torch device tensors, as dev_accept_blocks; d_connected (cap, 8)
        int64 or None. Returns the missing and the connected totals. Raises MvError with code
        E_INDEX_FULL when the reserved index or the reserved store (pending_reserve) has no room
        (both are unchanged)."""
        vp = ctypes.c_void_p
        nm, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
        n = d_off.shape[0] if d_off is not None else 0
        self._suspended = None  # the states stay on the device: connect_blocks asks pending_stats next time
        ptr = lambda t: vp(t.data_ptr()) if t is not None else None
        self._check(self.lib.mv_dev_connect_blocks(
            self.ctx, device, ptr(d_buf), int(buf_bytes), ptr(d_off), ptr(d_len), ptr(d_grp), n, ptr(d_blk_status),
            ptr(d_blk_state), ptr(d_missing), d_missing.shape[0] if d_missing is not None else 0, ctypes.byref(nm),
            ptr(d_connected), d_connected.shape[0] if d_connected is not None else 0, ctypes.byref(nc),
            vp(stream_handle or None)), "mv_dev_connect_blocks")
        return int(nm.value), int(nc.value)

    def pending_reserve(self, blocks: int, includes: int):
        """Room in the suspended-block store for `blocks` blocks with `includes` includes in all."""
        self._check(self.lib.mv_pending_reserve(self.ctx, int(blocks), int(includes)), "mv_pending_reserve")

    def pending_stats(self) -> "PendingStats":
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_pending_stats(self.ctx, _p(out)), "mv_pending_stats")
        self._suspended = int(out[1])
        return PendingStats(*(int(x) for x in out))

    def dag_reserve(self, blocks: int, includes: int):
        """Turns the DAG store on (mv_dag_reserve), with room for `blocks` records and `includes`
        includes in all: from now on connect_blocks keeps the edges of what it connects."""
        self._check(self.lib.mv_dag_reserve(self.ctx, int(blocks), int(includes)), "mv_dag_reserve")

    def dag_prune(self, round: int):
        """Drops the records of rounds below `round` (mv_dag_prune)."""
        self._check(self.lib.mv_dag_prune(self.ctx, int(round)), "mv_dag_prune")

    def dag_stats(self) -> "DagStats":
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_dag_stats(self.ctx, _p(out)), "mv_dag_stats")
        return DagStats(*(int(x) for x in out))

    def decide_leaders(self, leaders) -> "Decided":
        """The direct decision rule (mv_decide_leaders) for every (authority, round) of `leaders`."""
        rows = np.ascontiguousarray(np.asarray(leaders, dtype=np.uint64).reshape(-1, 2))
        n = rows.shape[0]
        out, stakes = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 3), dtype=np.uint64)
        self._check(self.lib.mv_decide_leaders(self.ctx, _p(rows) if n else None, n, _p(out) if n else None,
                                               _p(stakes) if n else None), "mv_decide_leaders")
        return Decided(out, stakes)

    def dev_decide_leaders(self, device: int, d_leaders, d_out, d_stakes=None, stream_handle: int = 0):
        """mv_dev_decide_leaders on torch device tensors: d_leaders (n, 2), d_out (n, 8), d_stakes
        (n, 3) or None, all int64."""
        vp = ctypes.c_void_p
        ptr = lambda t: vp(t.data_ptr()) if t is not None else None
        self._check(self.lib.mv_dev_decide_leaders(self.ctx, device, ptr(d_leaders), d_leaders.shape[0], ptr(d_out),
                                                   ptr(d_stakes), vp(stream_handle or None)), "mv_dev_decide_leaders")

    def commit_leaders(self, leaders) -> "Committed":
        """The direct and the indirect decision rule and the decided prefix (mv_commit_leaders) for the
        (authority, round) rows of `leaders`, which stand in sequence order: ascending round."""
        rows = np.ascontiguousarray(np.asarray(leaders, dtype=np.uint64).reshape(-1, 2))
        n = rows.shape[0]
        out, info = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        n_seq = ctypes.c_uint64(0)
        self._check(self.lib.mv_commit_leaders(self.ctx, _p(rows) if n else None, n, _p(out) if n else None,
                                               _p(info) if n else None, ctypes.byref(n_seq)), "mv_commit_leaders")
        return Committed(out, info, int(n_seq.value), rows)

    def dev_commit_leaders(self, device: int, d_leaders, d_out, d_info, stream_handle: int = 0) -> int:
        """mv_dev_commit_leaders on torch device tensors: d_leaders (n, 2), d_out (n, 8), d_info (n, 4),
        all int64. Returns the sequence's length."""
        vp = ctypes.c_void_p
        n_seq = ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_commit_leaders(self.ctx, device, vp(d_leaders.data_ptr()), d_leaders.shape[0],
                                                   vp(d_out.data_ptr()), vp(d_info.data_ptr()), ctypes.byref(n_seq),
                                                   vp(stream_handle or None)), "mv_dev_commit_leaders")
        return int(n_seq.value)

    def linearize(self, leaders, cap: int = 1 << 16) -> "Linearized":
        """The sub-DAGs of the committed leader blocks `leaders` ((n, 6) references in sequence order), in
        the reference's order (mv_linearize); at most `cap` blocks in all."""
        rows = ref_words(leaders)
        n, cap = rows.shape[0], int(cap)
        blocks, sub = np.zeros((max(cap, 1), 6), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        n_rows = ctypes.c_uint64(0)
        self._check(self.lib.mv_linearize(self.ctx, _p(rows) if n else None, n, _p(blocks) if cap else None, cap,
                                          _p(sub) if n else None, ctypes.byref(n_rows)), "mv_linearize")
        return Linearized(blocks[:int(n_rows.value)], sub, int(n_rows.value))

    def dev_linearize(self, device: int, d_leaders, d_blocks, d_sub, stream_handle: int = 0) -> int:
        """mv_dev_linearize on torch device tensors: d_leaders (n, 6), d_blocks (cap, 6), d_sub (n, 4), all
        int64. Returns the rows written."""
        vp = ctypes.c_void_p
        n_rows = ctypes.c_uint64(0)
        self._check(self.lib.mv_dev_linearize(self.ctx, device, vp(d_leaders.data_ptr()), d_leaders.shape[0],
                                              vp(d_blocks.data_ptr()), d_blocks.shape[0], vp(d_sub.data_ptr()),
                                              ctypes.byref(n_rows), vp(stream_handle or None)), "mv_dev_linearize")
        return int(n_rows.value)

    def linearize_mark(self, refs, height: int = 0):
        """Marks the references (n, 6) as committed and raises last_height to `height` (mv_linearize_mark)."""
        rows = ref_words(refs)
        n = rows.shape[0]
        self._check(self.lib.mv_linearize_mark(self.ctx, _p(rows) if n else None, n, int(height)), "mv_linearize_mark")

    def linearize_stats(self) -> "LinearStats":
        out = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.mv_linearize_stats(self.ctx, _p(out)), "mv_linearize_stats")
        return LinearStats(int(out[0]), int(out[1]))

    def propose_reserve(self, authority: int, entries: int = 0):
        """Opts in to the proposer's state for `authority` (mv_propose_reserve): the clock at round 0, an
        empty queue with room for `entries`."""
        self._check(self.lib.mv_propose_reserve(self.ctx, int(authority), int(entries)), "mv_propose_reserve")

    def propose_add(self, rows, tags=None, in_order: bool = False, payload: Optional[int] = None) -> "ProposeClock":
        """Core::add_blocks' loop over the processed blocks (mv_propose_add): rows (n, 6) references or
        (n, 8) connected rows as connect_blocks gives them, tags (n,) their WAL positions; payload: the
        token of the payload entry that follows them."""
        if isinstance(rows, np.ndarray) and rows.ndim == 2 and rows.shape[1] >= 6:
            rows = np.ascontiguousarray(rows, dtype=np.uint64)
        else:
            rows = ref_words(rows)  # (n, 6) words, or (authority, round, digest) tuples
        n, stride = rows.shape
        t = None if tags is None else np.ascontiguousarray(np.asarray(tags, dtype=np.uint64))
        if t is not None and t.shape != (n,):
            raise ValueError("tags: one word per row")
        flags = (PROPOSE_IN_ORDER if in_order else 0) | (PROPOSE_PAYLOAD if payload is not None else 0)
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_propose_add(self.ctx, _p(rows) if n else None, n, stride, _p(t) if n else None, flags,
                                            int(payload or 0), _p(out)), "mv_propose_add")
        return ProposeClock(*(int(x) for x in out))

    def dev_propose_add(self, device: int, d_rows, d_tags=None, in_order: bool = False, payload: Optional[int] = None,
                        n: Optional[int] = None, stream_handle: int = 0) -> "ProposeClock":
        """mv_dev_propose_add on torch device tensors: d_rows (>= n, stride) int64 with stride >= 6 (the
        first n rows; connected rows as dev_connect_blocks wrote them), d_tags (n,) int64 or None."""
        import torch

        vp = ctypes.c_void_p
        n = d_rows.shape[0] if n is None else int(n)
        flags = (PROPOSE_IN_ORDER if in_order else 0) | (PROPOSE_PAYLOAD if payload is not None else 0)
        d_out = torch.zeros(4, dtype=torch.int64, device=d_rows.device)
        self._check(self.lib.mv_dev_propose_add(self.ctx, device, vp(d_rows.data_ptr()), n, d_rows.shape[1],
                                                vp(d_tags.data_ptr()) if d_tags is not None else None, flags,
                                                int(payload or 0), vp(d_out.data_ptr()), vp(stream_handle or None)),
                    "mv_dev_propose_add")
        return ProposeClock(*(int(x) for x in d_out.cpu().numpy().view(np.uint64)))

    def propose_take(self, cap: int = 1 << 12, cap_payloads: int = 1 << 12) -> "Proposal":
        """Core::try_new_block's include choice (mv_propose_take): the includes without the own last
        block, the payload tokens, and the out words."""
        cap, cap_p = int(cap), int(cap_payloads)
        # one guard row / word behind each cap: the library writes nothing there (Proposal.guard_intact)
        inc = np.full((cap + 1, 6), PROPOSE_GUARD, dtype=np.uint64)
        pay = np.full(cap_p + 1, PROPOSE_GUARD, dtype=np.uint64)
        out = np.zeros(6, dtype=np.uint64)
        ni, npay = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.mv_propose_take(self.ctx, _p(inc) if cap else None, cap, ctypes.byref(ni),
                                             _p(pay) if cap_p else None, cap_p, ctypes.byref(npay), _p(out)),
                    "mv_propose_take")
        return Proposal(inc, pay, int(ni.value), int(npay.value), cap, cap_p, out)

    def propose_own(self, ref, includes=None) -> "ProposeClock":
        """The own block after it was sealed, or the own genesis block (mv_propose_own). includes None:
        the own last block followed by the outstanding take's choice; else the (k, 6) list, k may be 0."""
        r = ref_words(ref if isinstance(ref, np.ndarray) else [ref]).reshape(6)
        inc, k = None, 0
        if includes is not None:
            inc = ref_words(includes) if len(includes) else np.zeros((1, 6), dtype=np.uint64)
            k = len(includes)
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.mv_propose_own(self.ctx, _p(r), _p(inc), k, _p(out)), "mv_propose_own")
        return ProposeClock(*(int(x) for x in out))

    def propose_stats(self) -> "ProposeStats":
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.mv_propose_stats(self.ctx, _p(out)), "mv_propose_stats")
        return ProposeStats(*(int(x) for x in out))

    def dev_index_insert(self, device: int, d_words, stride_words: int, n: int, state: int = REF_HAVE,
                         stream_handle: int = 0, word_offset: int = 0):
        """mv_dev_index_insert: reference i is the six int64 words of torch device tensor d_words at
        word_offset + i * stride_words (a replay's rows: word_offset 3, stride 10). Enqueue only."""
        self._check(self.lib.mv_dev_index_insert(self.ctx, device, ctypes.c_void_p(d_words.data_ptr() + 8 * word_offset),
                                                 int(stride_words), int(n), int(state),
                                                 ctypes.c_void_p(stream_handle or None)), "mv_dev_index_insert")

    # ---- diagnostics ----
    def selftest(self, op: int, words: np.ndarray) -> np.ndarray:
        """Ops 0..63 take and return 16-word rows; ops >= SELFTEST_WIDE_OP (raw-limb field and point
        functions, kernels.hip k_selftest_wide; from 112 the scalar functions of scalar25519.h,
        k_selftest_scalar) take and return 64-word rows: `words` must be two-dimensional with that
        width."""
        width = 64 if op >= SELFTEST_WIDE_OP else 16
        w = np.asarray(words, dtype=np.uint32)
        if width == 64 and (w.ndim != 2 or w.shape[1] != 64):
            raise ValueError(f"selftest op {op} takes rows of 64 words, got shape {w.shape}")
        w = np.ascontiguousarray(w).reshape(-1, width)
        out = np.zeros_like(w)
        self._check(self.lib.mv_selftest(self.ctx, op, _p(w), w.shape[0], _p(out)), "mv_selftest")
        return out

    def batch_prep(self, msg, sig, pk=None, key_idx=None, groups: int = 1, secret: bytes = bytes(32), call: int = 0,
                   launch_sigs: int = 0) -> "BatchPrep":
        """The batch path's preparation stage alone (mv_selftest_batch_prep: k_bv_prep launched as
        a verify call launches it) with the coefficient key (secret, call) given. launch_sigs: 0 =
        one launch, else signatures per launch (a multiple of 256), as pinned inputs' copy chunks
        gate them. Returns a BatchPrep."""
        msg, sig = _u8(msg, 32), _u8(sig, 64)
        n = msg.shape[0]
        pk_a = _u8(pk, 32) if pk is not None else None
        ki = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32)) if key_idx is not None else None
        if len(secret) != 32:
            raise ValueError("secret: 32 bytes")
        key = np.frombuffer(bytes(secret) + int(call).to_bytes(8, "little"), dtype=np.uint8)
        scal = np.zeros((n, 12), dtype=np.uint32)
        pts = np.full((2 * n, 32), BATCH_PREP_UNWRITTEN, dtype=np.uint32)
        bsum = np.zeros((BATCH_MAX_GROUPS, 12), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        info = np.zeros(3, dtype=np.uint32)
        self._check(self.lib.mv_selftest_batch_prep(self.ctx, _p(msg), _p(sig), _p(pk_a), _p(ki), n, int(groups), _p(key),
                                                    int(launch_sigs), _p(scal), _p(pts), _p(bsum), _p(st), _p(info)),
                    "mv_selftest_batch_prep")
        return BatchPrep(scal, pts, bsum, st, int(info[0]), int(info[1]), bool(info[2]))

    def batch_msm(self, scal, pts, bsum, groups: int = 1, key_idx=None, n_keys: int = 0) -> "BatchMsm":
        """The batch path's stages after the preparation (mv_selftest_batch_msm: sort, buckets,
        per-key A term, reduction and k_bv_final, launched as a verify call launches them) on rows in
        BatchPrep's layout: scal (n, 12), pts (2 n, 32) -- (n, 32) will do with key_idx --, bsum
        (16, 12) uint64. key_idx / n_keys: the per-key form on the committee that is set. Returns a
        BatchMsm."""
        scal = np.ascontiguousarray(np.asarray(scal, dtype=np.uint32))
        n = scal.shape[0]
        pts = np.ascontiguousarray(np.asarray(pts, dtype=np.uint32))
        bsum = np.ascontiguousarray(np.asarray(bsum, dtype=np.uint64))
        ki = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32)) if key_idx is not None else None
        if scal.shape != (n, 12) or pts.shape not in ((2 * n, 32),) + (((n, 32),) if ki is not None else ()):
            raise ValueError("scal: (n, 12), pts: (2 n, 32)")
        if bsum.shape != (BATCH_MAX_GROUPS, 12) or (ki is not None and ki.shape != (n,)):
            raise ValueError("bsum: (16, 12), key_idx: (n,)")
        win = np.zeros((BATCH_MAX_GROUPS * 16, 36), dtype=np.uint32)
        asum = np.zeros((BATCH_MAX_GROUPS, 36), dtype=np.uint32)
        flags = np.zeros(1 + BATCH_MAX_GROUPS, dtype=np.uint32)
        info = np.zeros(3, dtype=np.uint32)
        self._check(self.lib.mv_selftest_batch_msm(self.ctx, n, int(groups), _p(scal), _p(pts), _p(bsum), _p(ki),
                                                   int(n_keys), _p(win), _p(asum), _p(flags), _p(info)),
                    "mv_selftest_batch_msm")
        g, nw = int(info[0]), int(info[2])
        return BatchMsm(win[:g * nw].reshape(g, nw, 36) if g else win[:0].reshape(0, 0, 36),
                        asum[:g] if ki is not None else None, int(flags[0]), [int(f) for f in flags[1:1 + g]], g,
                        int(info[1]))

    def comb_table(self, key: Optional[int] = None) -> np.ndarray:
        """One radix-256 comb table as it stands on device 0 (mv_selftest_comb_table): the base
        point's (key None) or committee key `key`'s, which holds the multiples of -A. Returns
        (32, 129, 32) uint32: entry [i][j] = [j 256^i]P as (y+x, y-x, 2dxy) in 9 canonical 29-bit
        limbs each, then 5 zero words."""
        out = np.zeros((COMB_ROWS, COMB_ENTRIES, 32), dtype=np.uint32)
        self._check(self.lib.mv_selftest_comb_table(self.ctx, -1 if key is None else int(key), _p(out)),
                    "mv_selftest_comb_table")
        return out


def _pack(blocks: Sequence[bytes]):
    lens = np.array([len(b) for b in blocks], dtype=np.uint64)
    offs = np.zeros(len(blocks), dtype=np.uint64)
    if len(blocks) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    return np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8), offs, lens


def ref_words(refs) -> np.ndarray:
    """(n, 6) uint64 index keys -- authority, round, the four little-endian digest words -- from
    such an array or from (authority, round, 32-byte digest) tuples (blocks.genesis_refs)."""
    if isinstance(refs, np.ndarray):
        return np.ascontiguousarray(refs, dtype=np.uint64).reshape(-1, 6)
    out = np.zeros((len(refs), 6), dtype=np.uint64)
    for i, (a, r, d) in enumerate(refs):
        out[i, 0], out[i, 1] = a, r
        out[i, 2:] = np.frombuffer(bytes(d), dtype="<u8")
    return out


def block_preimage(bincode: bytes) -> Optional[bytes]:
    """Host-side pre-image of one bincode StatementBlock (None if it does not deserialize)."""
    lib = load_library()
    b = np.frombuffer(bincode + b"\0", dtype=np.uint8)
    n = lib.mv_block_preimage(_p(b), len(bincode), None, 0)
    if n < 0:
        return None
    out = np.zeros(max(n, 1), dtype=np.uint8)
    lib.mv_block_preimage(_p(b), len(bincode), _p(out), n)
    return out[:n].tobytes()


def shard_plan(weights, parts: int) -> List[int]:
    """Host-only: the contiguous shard cuts the multi-device paths use (balanced by weight)."""
    lib = load_library()
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.uint64))
    cut = np.zeros(parts + 1, dtype=np.uint64)
    rc = lib.mv_shard_plan(_p(w) if w.size else None, w.size, parts, _p(cut))
    if rc != MV_OK:
        raise MvError(f"mv_shard_plan failed ({rc})")
    return [int(c) for c in cut]


def wal_layout(payload_lens, map_bits: int = WAL_MAP_BITS, start: int = 0):
    """Host-only: WalWriter::writev positions of entries with these payload lengths, and the
    writer position after them."""
    lib = load_library()
    pl = np.ascontiguousarray(np.asarray(payload_lens, dtype=np.uint64))
    pos = np.zeros(max(pl.size, 1), dtype=np.uint64)
    end = lib.mv_wal_layout(_p(pl) if pl.size else None, pl.size, map_bits, start, _p(pos))
    return pos[:pl.size], int(end)


def frame_blocks(buf) -> Tuple[np.ndarray, np.ndarray, int]:
    """Host-only: (offsets, lengths) of the Data<StatementBlock> byte strings inside received
    NetworkMessage frames (mv_frame_blocks, network.rs:400-447), and the bytes of the complete
    frames. Raises MvError where the reference would drop the connection."""
    lib = load_library()
    b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf,
                             dtype=np.uint8)
    consumed = ctypes.c_uint64(0)
    n = lib.mv_frame_blocks(_p(b) if b.size else None, b.size, None, None, 0, ctypes.byref(consumed))
    if n < 0:
        raise MvError("mv_frame_blocks: a malformed frame stream (the reference drops the connection)")
    offs = np.zeros(max(n, 1), dtype=np.uint64)
    lens = np.zeros(max(n, 1), dtype=np.uint64)
    lib.mv_frame_blocks(_p(b) if b.size else None, b.size, _p(offs), _p(lens), n, ctypes.byref(consumed))
    return offs[:n], lens[:n], int(consumed.value)


class BatchPrep:
    """Result of Engine.batch_prep (include/mysti_verify.h, mv_selftest_batch_prep). scal: (n, 12)
    uint32, z_i in words 0..3 and z_i k_i mod l in words 4..11; pts: (2 n, 32) uint32 limb rows (27
    words: y+x, y-x, 2dxy), R at i and A at n + i (BATCH_PREP_UNWRITTEN words where a_rows is
    False); bsum: (16, 12) uint64 column sums of z_i s_i per group; status: MV_SIG_* per signature;
    groups, group_sigs: the geometry the engine used."""

    def __init__(self, scal, pts, bsum, status, groups, group_sigs, a_rows):
        self.scal, self.pts, self.bsum, self.status = scal, pts, bsum, status
        self.groups, self.group_sigs, self.a_rows = groups, group_sigs, a_rows

    def z(self, i: int) -> int:
        return int.from_bytes(self.scal[i, :4].tobytes(), "little")

    def zk(self, i: int) -> int:
        return int.from_bytes(self.scal[i, 4:].tobytes(), "little")

    def group_sum(self, g: int) -> int:
        """sum z_i s_i over group g, from its 12 columns (each a sum of 32-bit words)."""
        return sum(int(c) << (32 * k) for k, c in enumerate(self.bsum[g]))


class BatchMsm:
    """Result of Engine.batch_msm (include/mysti_verify.h, mv_selftest_batch_msm). win: (groups, nw,
    36) uint32, the extended point (X, Y, Z, T, 9 limbs each) of every group's window sum as
    k_bv_final read it (nw = 16, or 8 in the per-key form); asum: (groups, 36) per-key A terms or
    None; flag_all and flags[g]: the equation held; groups, group_sigs: the geometry used."""

    def __init__(self, win, asum, flag_all, flags, groups, group_sigs):
        self.win, self.asum, self.flag_all, self.flags = win, asum, flag_all, flags
        self.groups, self.group_sigs = groups, group_sigs


class IndexStats:
    """Result of Engine.index_stats (mv_index_stats): HAVE and WANTED entries, the capacity in
    entries, rebuilds so far, the longest probe since the last clear."""

    def __init__(self, have, wanted, capacity, rebuilds, longest_probe):
        self.have, self.wanted, self.capacity = have, wanted, capacity
        self.rebuilds, self.longest_probe = rebuilds, longest_probe


class VotesStats:
    """Result of Engine.votes_stats (mv_votes_stats): pending sharing blocks
    (TransactionAggregator::len), aggregating cells, cells of capacity in use, transactions
    certified since create / clear."""

    def __init__(self, pending, aggregating, cells_in_use, certified):
        self.pending, self.aggregating, self.cells_in_use, self.certified = pending, aggregating, cells_in_use, certified

    def as_tuple(self):
        return (self.pending, self.aggregating, self.cells_in_use, self.certified)


class Accepted:
    """Result of Engine.accept_blocks (include/mysti_verify.h, mv_accept_blocks). blk_status: MV_BLOCK_*
    per block (BLOCK_OK for blocks skipped as known); blk_state: ACC_* per block; missing: (k, 6)
    uint64 references seen missing for the first time, in (block, include) order; n_missing: their
    total (above k when cap_missing cut the list)."""

    def __init__(self, blk_status, blk_state, missing, n_missing):
        self.blk_status, self.blk_state, self.missing, self.n_missing = blk_status, blk_state, missing, n_missing


class Connected(Accepted):
    """Result of Engine.connect_blocks (mv_connect_blocks): Accepted, and connected: (k, 8) uint64
    rows -- the reference, the block's index in the call or CONNECT_EARLIER, its level -- in causal
    order; n_connected: their total (above k when cap_connected cut the list)."""

    def __init__(self, blk_status, blk_state, missing, n_missing, connected, n_connected):
        super().__init__(blk_status, blk_state, missing, n_missing)
        self.connected, self.n_connected = connected, n_connected


class PendingStats:
    """Result of Engine.pending_stats (mv_pending_stats): REF_STORED entries, suspended blocks,
    their includes, the levels of the last connect call."""

    def __init__(self, stored, suspended, includes, levels):
        self.stored, self.suspended, self.includes, self.levels = stored, suspended, includes, levels


class DagStats:
    """Result of Engine.dag_stats (mv_dag_stats): records, their includes, the lowest and the
    highest round of a record."""

    def __init__(self, records, includes, lowest_round, highest_round):
        self.records, self.includes, self.lowest_round, self.highest_round = records, includes, lowest_round, highest_round


class Linearized:
    """Result of Engine.linearize (mv_linearize): blocks (n_rows, 6) uint64, the sub-DAGs one behind the
    other; sub (n, 4) uint64 -- LINEAR_* status, first row, count, height; n_rows."""

    def __init__(self, blocks, sub, n_rows):
        self.blocks, self.sub, self.n_rows = blocks, sub, n_rows
        self.status = sub[:, 0].astype(np.int64)

    def sub_dag(self, i):
        """The blocks of leader i, as tuples of six words."""
        first, count = int(self.sub[i, 1]), int(self.sub[i, 2])
        return [tuple(int(w) for w in row) for row in self.blocks[first:first + count]]


class LinearStats:
    """Result of Engine.linearize_stats (mv_linearize_stats): the marked references and last_height."""

    def __init__(self, marked, last_height):
        self.marked, self.last_height = marked, last_height


class ProposeClock:
    """Result of Engine.propose_add / propose_own: the clock round after the call, the aggregator's stake
    and voters, the queue's length."""

    def __init__(self, round, stake, voters, queue):
        self.round, self.stake, self.voters, self.queue = round, stake, voters, queue

    def words(self):
        return [self.round, self.stake, self.voters, self.queue]


class Proposal:
    """Result of Engine.propose_take (mv_propose_take): proposed, round (the clock's: the new block's),
    taken (queue entries), flags (PROPOSE_*), next_entry (the tag of the first entry left,
    PROPOSE_NO_ENTRY without one), queue (its length); includes (min(n_includes, cap), 6) uint64 without
    the own last block, payloads the tokens; n_includes and n_payloads are the totals."""

    def __init__(self, inc, pay, n_includes, n_payloads, cap, cap_p, out):
        self.n_includes, self.n_payloads = n_includes, n_payloads
        self.includes, self.payloads = inc[:min(n_includes, cap)], pay[:min(n_payloads, cap_p)]
        # nothing was written past what the call filled, nor past the caps
        self.guard_intact = bool((inc[min(n_includes, cap):] == PROPOSE_GUARD).all() and
                                 (pay[min(n_payloads, cap_p):] == PROPOSE_GUARD).all())
        self.proposed, self.round, self.taken, self.flags, self.next_entry, self.queue = (int(x) for x in out)

    def include_refs(self):
        """The includes as tuples of six words."""
        return [tuple(int(w) for w in row) for row in self.includes]


class ProposeStats:
    """Result of Engine.propose_stats (mv_propose_stats)."""

    def __init__(self, round, stake, voters, queue, own_round, outstanding, takes, dropped):
        self.round, self.stake, self.voters, self.queue = round, stake, voters, queue
        self.own_round, self.outstanding, self.takes, self.dropped = own_round, outstanding, takes, dropped

    def words(self):
        return [self.round, self.stake, self.voters, self.queue, self.own_round, self.outstanding, self.takes, self.dropped]


class Seeded:
    """What a seed call did (mv_wal_recover, mv_dev_dag_seed_rows): the rows whose references rose to
    REF_STORED, the records appended to the DAG store and their includes, the includes entered as
    REF_WANTED (0 for a self-contained WAL), and the OK rows whose bytes did not fit the image."""

    def __init__(self, rows, records, includes, wanted, misfits):
        self.rows, self.records, self.includes, self.wanted, self.misfits = rows, records, includes, wanted, misfits

    def words(self):
        return [self.rows, self.records, self.includes, self.wanted, self.misfits]


class Decided:
    """Result of Engine.decide_leaders (mv_decide_leaders): rows (n, 8) uint64 -- words 0-5 the
    committed reference, 6 the LEADER_* status, 7 the leader blocks found -- and stakes (n, 3):
    blame, vote and certificate stake."""

    def __init__(self, rows, stakes):
        self.rows, self.stakes = rows, stakes
        self.status = rows[:, 6].astype(np.int64)
        self.leader_blocks = rows[:, 7].astype(np.int64)

    def ref(self, i: int):
        """(authority, round, digest) of row i's committed block, None unless LEADER_COMMIT."""
        if int(self.rows[i, 6]) != LEADER_COMMIT:
            return None
        return int(self.rows[i, 0]), int(self.rows[i, 1]), self.rows[i, 2:6].astype("<u8").tobytes()


class Committed(Decided):
    """Result of Engine.commit_leaders (mv_commit_leaders): rows as Decided's; info (n, 4) uint64 --
    the COMMIT_KIND_*, the anchor's row or COMMIT_NO_ANCHOR, the COMMIT_INCOMPLETE / COMMIT_BLOCKED
    bits, the records the walk reached in the decision round -- and n_sequence, the length of the
    decided prefix over the rows of round > 0. leaders: the (n, 2) rows the call was given."""

    def __init__(self, rows, info, n_sequence, leaders):
        super().__init__(rows, None)
        self.info, self.n_sequence, self.leaders = info, n_sequence, leaders
        self.kind, self.flags = info[:, 0].astype(np.int64), info[:, 2].astype(np.int64)

    def sequence(self):
        """The decided rows, in order: (row, status)."""
        rows = [i for i in range(self.leaders.shape[0]) if int(self.leaders[i, 1]) > 0][:self.n_sequence]
        return [(i, int(self.status[i])) for i in rows]


@dataclasses.dataclass
class WalWrite:
    """Result of Engine.wal_write (include/mysti_verify.h, mv_wal_write). image: the bytes to append
    at the writer position the call was given (uint8; empty when they did not fit the cap); pos: the
    WalPosition.start of every entry; end_pos: the writer position after them."""
    image: np.ndarray
    pos: np.ndarray
    end_pos: int


class WalReplay:
    """Result of Engine.wal_replay (include/mysti_verify.h, mv_wal_replay). pos / tag / len / status:
    the entries in iteration order; rows: (n, 10) uint64 block rows (entry index, offset and length
    of the block's bincode, authority, round, the four digest words, next_entry or WAL_NONE);
    blk_status: MV_BLOCK_* per row; summary: highest_round, last own row, last state entry (or
    WAL_NONE); last_seen: per authority. count / n_blocks: the totals (above the array lengths when
    a cap cut them)."""

    def __init__(self, pos, tag, len, status, rows, blk_status, summary, last_seen, count, n_blocks):
        self.pos, self.tag, self.len, self.status = pos, tag, len, status
        self.rows, self.blk_status, self.summary, self.last_seen = rows, blk_status, summary, last_seen
        self.count, self.n_blocks = count, n_blocks

    @property
    def digests(self) -> np.ndarray:
        """(n, 32) uint8: the stored digest of every row's block."""
        return np.ascontiguousarray(self.rows[:, 5:9]).view(np.uint8).reshape(-1, 32)


class FrameVerdicts:
    """Result of Engine.verify_frames_messages / frame_messages. rows: (n, 8) uint32 message rows
    (include/mysti_verify.h: stream, tag, off low / high, first_block, n_blocks,
    status | bad_status << 8, bad_block); consumed and drop_msg per stream; blk_off / blk_len /
    blk_status per listed block (blk_status is None for the host-only walk)."""

    def __init__(self, rows, consumed, drop_msg, blk_off, blk_len, blk_status):
        self.rows, self.consumed, self.drop_msg = rows, consumed, drop_msg
        self.blk_off, self.blk_len, self.blk_status = blk_off, blk_len, blk_status

    @property
    def status(self) -> np.ndarray:
        return self.rows[:, 6] & 0xFF

    @property
    def bad_status(self) -> np.ndarray:
        return (self.rows[:, 6] >> 8) & 0xFF

    @property
    def off(self) -> np.ndarray:
        return self.rows[:, 2].astype(np.uint64) | (self.rows[:, 3].astype(np.uint64) << np.uint64(32))


def frame_messages(buf) -> FrameVerdicts:
    """Host-only: the message rows of one stream of received frames (mv_frame_messages: the walk
    of mv_verify_frames with the statuses the bytes alone decide) and the blocks they list."""
    lib = load_library()
    b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf,
                             dtype=np.uint8)
    pb = _p(b) if b.size else None
    consumed, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    n = lib.mv_frame_messages(pb, b.size, None, 0, None, None, 0, ctypes.byref(nb), ctypes.byref(consumed))
    if n < 0:
        raise MvError("mv_frame_messages: bad arguments")
    rows = np.zeros((max(n, 1), 8), dtype=np.uint32)
    offs = np.zeros(max(nb.value, 1), dtype=np.uint64)
    lens = np.zeros(max(nb.value, 1), dtype=np.uint64)
    lib.mv_frame_messages(pb, b.size, _p(rows), n, _p(offs), _p(lens), nb.value, ctypes.byref(nb),
                          ctypes.byref(consumed))
    drop = np.array([next((i for i in range(n) if rows[i, 6] & 0xFF), MSG_NONE)], dtype=np.uint32)
    return FrameVerdicts(rows[:n], np.array([consumed.value], dtype=np.uint64), drop, offs[:nb.value],
                         lens[:nb.value], None)


def version() -> str:
    return load_library().mv_version().decode()
