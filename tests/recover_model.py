"""Helper (not a test): what mv_wal_recover / mv_dev_dag_seed_rows do with the rows of a replay,
restated in plain Python over the rows of replay_model.model, for tests/test_recover_model.py (hand-
written images) and tests/test_gpu_recover.py (which holds the library to it). The wording followed
is include/mysti_verify.h's (mv_wal_recover, steps 1-3): BlockStore::open with add_unloaded
(block_store.rs:50-116, 398-404) as what makes a replayed block visible to BaseCommitter.

  Store.seed   1. every row's reference is STORED, whatever its verdict
               2. a row gets a record when its verdict is OK, its round >= floor, it is the first
                  row of the call with its reference and that reference has no record, and its
                  bincode fits the image (an OK row that does not fit is a misfit)
               3. the includes of a record row with no entry become WANTED, each once
  Store.rule   a commit_seq_model.CommitRule fed with exactly the records, in order

The includes are read with struct.unpack from the image. Nothing here is shared with the library's
kernels."""
import struct

import commit_seq_model as S

BLOCK_OK = 0
WANTED, HAVE, STORED = 1, 2, 3


def _ref(words):
    a, r, *d = (int(w) for w in words)
    return (a, r, struct.pack("<4Q", *d))


def row_includes(raw, off, length):
    """The includes of the block raw[off, off + length), or None when its bytes do not fit."""
    if length < 64 or off + length > len(raw):
        return None
    k = struct.unpack_from("<Q", raw, off + 56)[0]
    if 64 + 56 * k > length:
        return None
    out = []
    for j in range(k):
        a, r, _ = struct.unpack_from("<QQQ", raw, off + 64 + 56 * j)
        out.append((a, r, bytes(raw[off + 88 + 56 * j:off + 120 + 56 * j])))
    return out


class Store:
    """The references with a state, and the DAG store's records in order: [(reference, includes)]."""

    def __init__(self, stored=()):
        self.state = {r: STORED for r in stored}
        self.records = []

    def add_record(self, ref, includes):
        """A record from elsewhere (a connect call's row)."""
        self.state[ref] = STORED
        self.records.append((ref, list(includes)))

    def seed(self, image, rows, blk_status, floor=0):
        """One seed call over rows (n x 10) and their verdicts -> the five words of `seeded`."""
        raw = bytes(image)
        had = {ref for ref, _ in self.records}
        seen, new, misfits = set(), [], 0
        for row, st in zip(rows, blk_status):
            ref = _ref(row[3:9])
            self.state[ref] = STORED
            first = ref not in seen
            seen.add(ref)
            if int(st) != BLOCK_OK:
                continue
            incs = row_includes(raw, int(row[1]), int(row[2]))
            if incs is None:
                misfits += 1
                continue
            if int(row[4]) >= floor and first and ref not in had:
                new.append((ref, incs))
        wanted = 0
        for _, incs in new:
            for i in incs:
                if i not in self.state:
                    self.state[i] = WANTED
                    wanted += 1
        self.records += new
        return [len(rows), len(new), sum(len(i) for _, i in new), wanted, misfits]

    def prune(self, floor):
        self.records = [(r, i) for r, i in self.records if r[1] >= floor]

    def wanted(self):
        return {r for r, s in self.state.items() if s == WANTED}

    def stored(self):
        return {r for r, s in self.state.items() if s == STORED}

    def stats(self):
        """mv_dag_stats: records, includes, lowest and highest round."""
        rounds = [r[1] for r, _ in self.records]
        return (len(self.records), sum(len(i) for _, i in self.records), min(rounds, default=0), max(rounds, default=0))

    def rule(self, stakes):
        d = S.CommitRule(stakes)
        for ref, incs in self.records:
            d.add(ref, incs)
        return d
