"""Helper (not a test): the replay loop of BlockStore::open (block_store.rs:50-116) restated in plain
Python for the tests of mv_wal_replay / mv_dev_wal_replay.

  the iteration        oracle.wal_iter (WalReader::iter_until, wal.rs:226-346): entries in order,
                       the last one failing where try_read panics
  the tag match        block_store.rs:71-99: tags 1..5, anything else panics (:98)
  the decode           tag 1: Data::<StatementBlock>::from_bytes (:73-74); tag 3: OwnBlockData's u64
                       next_entry, then the block (:83-84, 526-540)
  the index            add_unloaded with the block's own BlockReference, highest_round and
                       last_seen_by_authority, whose expect panics on an authority outside the
                       committee (:398-404, 424-432)
  the builder          RecoveredStateBuilder: the last own block, the last state entry (state.rs:39-59)

Whether a block decodes, and what StatementBlock::verify says of it, comes from `verdicts` (the
tests pass the CPU oracle's block_verify_batch, or a stand-in where they have no signed blocks);
the reference is read with struct.unpack from the block's first 56 bytes. Nothing here is shared
with the library's kernels. The result has the C ABI's layout (include/mysti_verify.h)."""
import struct

import numpy as np

import oracle as O

OK, CRC_MISMATCH, NONZERO_CRC_LEN0, BAD_LENGTH, UNKNOWN_TAG, BLOCK_DECODE, UNKNOWN_AUTHORITY = range(7)
TAG_BLOCK, TAG_PAYLOAD, TAG_OWN_BLOCK, TAG_STATE, TAG_COMMIT = 1, 2, 3, 4, 5
NONE = 0xFFFFFFFFFFFFFFFF
REF_BYTES = 56


def oracle_verdicts(pks, stakes, epoch):
    """verdicts(img, offs, lens) from the CPU oracle's StatementBlock::verify."""
    def fn(img, offs, lens):
        if not len(offs):
            return np.zeros(0, dtype=np.uint8)
        return O.block_verify_batch(np.concatenate([img, np.zeros(1, np.uint8)]), offs, lens, pks, stakes, epoch)[0]

    return fn


class Result:
    def __init__(self, pos, tag, ln, status, rows, blk_status, summary, last_seen):
        self.pos, self.tag, self.len, self.status = pos, tag, ln, status
        self.rows, self.blk_status, self.summary, self.last_seen = rows, blk_status, summary, last_seen
        self.count, self.n_blocks = pos.shape[0], rows.shape[0]


def model(image, end_pos, map_bits, n_auth, verdicts) -> Result:
    """The expected result of mv_wal_replay(image, end_pos, map_bits) for a committee of n_auth."""
    raw = bytes(image)
    img = np.frombuffer(raw, dtype=np.uint8)
    pos, tag, ln, st = (a.copy() for a in O.wal_iter(img, end_pos, map_bits))
    # the blocks of every tag-1 / tag-3 entry that has one, verified in one oracle call
    cand = {}
    for i in range(len(pos)):
        p, t, l = int(pos[i]), int(tag[i]), int(ln[i])
        skip = 8 if t == TAG_OWN_BLOCK else 0
        # (a payload that reaches past the file is the mapping's zero tail: the library reads no
        # block there and calls it a decode failure, include/mysti_verify.h)
        if st[i] == OK and t in (TAG_BLOCK, TAG_OWN_BLOCK) and l >= skip and p + 16 + l <= len(raw):
            cand[i] = (p + 16 + skip, l - skip)
    idx = sorted(cand)
    vs = verdicts(img, np.array([cand[i][0] for i in idx], dtype=np.uint64),
                  np.array([cand[i][1] for i in idx], dtype=np.uint64))
    verdict = dict(zip(idx, (int(v) for v in vs)))
    rows, blk_status, count = [], [], len(pos)
    highest, last_own, last_state, seen = 0, NONE, NONE, [0] * n_auth
    for i in range(len(pos)):
        p, t = int(pos[i]), int(tag[i])
        if st[i] == OK:
            if not TAG_BLOCK <= t <= TAG_COMMIT:
                st[i] = UNKNOWN_TAG
            elif t in (TAG_BLOCK, TAG_OWN_BLOCK):
                if i not in cand or verdict[i] == O.BLOCK_PARSE_ERROR:
                    st[i] = BLOCK_DECODE
                else:
                    off, blen = cand[i]
                    assert blen >= REF_BYTES  # a block that parses holds its own reference
                    authority, rnd, dlen = struct.unpack_from("<QQQ", raw, off)
                    assert dlen == 32
                    if authority >= n_auth:
                        st[i] = UNKNOWN_AUTHORITY
                    else:
                        nxt = struct.unpack_from("<Q", raw, off - 8)[0] if t == TAG_OWN_BLOCK else NONE
                        if t == TAG_OWN_BLOCK:
                            last_own = len(rows)
                        rows.append([i, off, blen, authority, rnd, *struct.unpack_from("<4Q", raw, off + 24), nxt])
                        blk_status.append(verdict[i])
                        highest = max(highest, rnd)
                        seen[authority] = max(seen[authority], rnd)
            elif t == TAG_STATE:
                last_state = i
        if st[i] != OK:  # the reference panics here
            count = i + 1
            break
    return Result(pos[:count], tag[:count], ln[:count], st[:count],
                  np.array(rows, dtype=np.uint64).reshape(-1, 10), np.array(blk_status, dtype=np.uint8),
                  np.array([highest, last_own, last_state], dtype=np.uint64), np.array(seen, dtype=np.uint64))


def assert_same(got, want, what=""):
    """got (mysticeti_amd.WalReplay, or anything with its fields) equals the model's Result."""
    assert (got.count, got.n_blocks) == (want.count, want.n_blocks), (what, got.count, got.n_blocks, want.count, want.n_blocks)
    for f in ("pos", "tag", "len", "status", "blk_status", "summary", "last_seen"):
        g, w = np.asarray(getattr(got, f)), getattr(want, f)
        assert g.tolist() == w.tolist(), (what, f, g.tolist()[:12], w.tolist()[:12])
    assert got.rows.shape == want.rows.shape, (what, got.rows.shape, want.rows.shape)
    bad = np.flatnonzero((np.asarray(got.rows) != want.rows).any(axis=1))
    assert not len(bad), (what, int(bad[0]), got.rows[bad[0]].tolist(), want.rows[bad[0]].tolist())
