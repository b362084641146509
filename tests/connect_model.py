"""Helper (not a test): what mv_connect_blocks computes, restated in plain Python over dicts and
lists, for tests/test_connect_model.py (which holds it to index_model.Reference, BlockManager's own
structures) and tests/test_gpu_connect.py (which holds the library to it).

  ThreeState    include/mysti_verify.h: one dict reference -> MV_REF_WANTED / HAVE / STORED, the
                suspended-block store as a list of records in arrival order, the five steps of an
                accept call (with KNOWN read as HAVE or STORED) and the sweep of step 6.
  Reference3    index_model.Reference with an accept that also returns add_blocks' first value,
                newly_blocks_processed.

Nothing here is shared with the library's kernels."""
import index_model as IM
from index_model import ABSENT, BLOCK_OK, DROPPED, DUP, HAVE, KNOWN, NEW, REJECTED, WANTED  # noqa: F401

STORED = 3
SUSPENDED = 5
EARLIER = 0xFFFFFFFFFFFFFFFF  # word 6 of a row: an earlier call suspended the block


class Connected(IM.Accepted):
    def __init__(self, blk_status, blk_state, missing, rows, levels):
        super().__init__(blk_status, blk_state, missing)
        self.rows, self.n_connected, self.levels = rows, len(rows), levels  # rows: (ref, index or EARLIER, level)


class ThreeState(IM.TwoState):
    """seed: the state the genesis references get (a caller that wants the cascade seeds STORED)."""

    def __init__(self, verdicts, genesis=(), seed=STORED):
        super().__init__(verdicts, ())
        self.state = {r: seed for r in genesis}
        self.pending = []  # records [reference, includes, index in the running call or EARLIER], arrival order
        self.levels = 0

    def counts(self):
        """(HAVE or STORED, WANTED): what mv_index_stats counts."""
        v = list(self.state.values())
        return sum(s >= HAVE for s in v), v.count(WANTED)

    def stored(self):
        return {r for r, s in self.state.items() if s == STORED}

    def have_only(self):
        return {r for r, s in self.state.items() if s == HAVE}

    def stats(self):
        """mv_pending_stats."""
        return (len(self.stored()), len(self.pending), sum(len(p[1]) for p in self.pending), self.levels)

    def accept(self, blocks, groups=None):
        """Steps 1-5 (mv_accept_blocks on this context): KNOWN is HAVE or STORED; nothing is parked."""
        n = len(blocks)
        refs = [IM.own_ref(b) for b in blocks]
        known = [r is not None and self.lookup(r) >= HAVE for r in refs]  # 1. probe
        todo = [i for i in range(n) if not known[i]]
        status = [BLOCK_OK] * n  # 2. verify
        for i, v in zip(todo, IM.run_verdicts(self.verdicts, [blocks[i] for i in todo])):
            status[i] = v
        state = [KNOWN if known[i] else (REJECTED if status[i] != BLOCK_OK else NEW) for i in range(n)]
        for lo, hi in IM.group_slices(n, groups):  # 3. groups
            if any(state[i] == REJECTED for i in range(lo, hi)):
                for i in range(lo, hi):
                    if state[i] == NEW:
                        state[i] = DROPPED
        seen = set()  # 4. own references
        for i in range(n):
            if state[i] == NEW:
                if refs[i] in seen:
                    state[i] = DUP
                else:
                    seen.add(refs[i])
                    self.state[refs[i]] = max(self.lookup(refs[i]), HAVE)
        missing = []  # 5. includes
        for i in range(n):
            if state[i] == NEW:
                for inc in IM.includes(blocks[i]):
                    if self.lookup(inc) == ABSENT:
                        self.state[inc] = WANTED
                        missing.append(inc)
        return IM.Accepted(status, state, missing)

    def connect(self, blocks=(), groups=None) -> Connected:
        blocks = list(blocks)
        acc = self.accept(blocks, groups)
        for i, b in enumerate(blocks):  # 6. the NEW blocks join the store in block order
            if acc.blk_state[i] == NEW:
                self.pending.append([IM.own_ref(b), IM.includes(b), i])
        rows, level = [], 0
        while True:  # level by level: the check of a level reads the states before the level
            hit = [p for p in self.pending
                   if self.lookup(p[0]) != STORED and all(self.lookup(i) == STORED for i in p[1])]
            if not hit:
                break
            for p in hit:
                rows.append((p[0], p[2], level))
            for p in hit:
                self.state[p[0]] = STORED
            level += 1
        self.levels = level
        self.pending = [p for p in self.pending if self.lookup(p[0]) != STORED]  # stable
        for p in self.pending:
            if p[2] != EARLIER:
                acc.blk_state[p[2]] = SUSPENDED
            p[2] = EARLIER
        return Connected(acc.blk_status, acc.blk_state, acc.missing, rows, level)


class Reference3(IM.Reference):
    def accept3(self, blocks, groups=None):
        """-> (`processed` per block, newly_blocks_processed, the missing references)."""
        refs = [IM.own_ref(b) for b in blocks]
        processed = [r is not None and self.exists_or_pending(r) for r in refs]
        todo = [i for i in range(len(blocks)) if not processed[i]]
        verdict = dict(zip(todo, IM.run_verdicts(self.verdicts, [blocks[i] for i in todo])))
        to_process = []
        for lo, hi in IM.group_slices(len(blocks), groups):
            mine = [i for i in range(lo, hi) if not processed[i]]
            if all(verdict[i] == BLOCK_OK for i in mine):
                to_process += [blocks[i] for i in mine]
        newly, missing = self.add_blocks(to_process) if to_process else ([], set())
        return processed, newly, missing


def rows_words(rows):
    """Rows as the (k, 8) uint64 array mv_connect_blocks writes."""
    import numpy as np

    out = np.zeros((len(rows), 8), dtype=np.uint64)
    if rows:
        out[:, :6] = IM.ref_words([r[0] for r in rows])
        out[:, 6] = [r[1] for r in rows]
        out[:, 7] = [r[2] for r in rows]
    return out
