"""Two statements of TransactionAggregator::process_block (committee.rs:263-482), for the tests of
mv_aggregate_votes.

VerbatimAggregator restates the reference as it is written: RangeMap::mutate_range
(range_map.rs:33-136) with its splits and its removal of emptied entries, StakeAggregator::add
(committee.rs:314-320), register / vote / process_block (:364-425, :450-481) and a handler that
records processed / duplicate / unknown. CellRule is the per-cell rule of include/mysti_verify.h.

Removing a sharing block from `pending` once its range map is empty (committee.rs:416-418) and
leaving its cells empty cannot be told apart afterwards: a later vote finds no entry either way
(unknown), and a later register starts from empty cells either way. test_votes_model.py holds the
two models against each other on exactly this, len() included.

Both take blocks as (author, ref, statements) (votes_cases.py) and return per block a Result:
processed [(ref, offset)] in order, unknown and duplicate counts, flag bits. The two inputs the
reference does not survive -- Vote::Reject (unimplemented!()) and a Vote at offset 2^64 - 1 (one()
overflows) -- are ignored and flagged in both, as are ranges verify rejects (end < start,
end - start >= 2^20).
"""
import bisect
from collections import namedtuple

FLAG_REJECT, FLAG_OFFSET, FLAG_RANGE, FLAG_REF_REUSED = 1, 2, 4, 8
U64 = (1 << 64) - 1
MAX_RANGE = 1 << 20

Result = namedtuple("Result", "processed unknown duplicate flags")


def quorum_threshold(stakes) -> int:
    return 2 * sum(stakes) // 3 + 1


def shared_ranges(statements):
    """types.rs:238-254: maximal runs of Share statements as [start, end)."""
    out, start = [], None
    for k, st in enumerate(statements):
        if st[0] == "share":
            if start is None:
                start = k
        elif start is not None:
            out.append((start, k))
            start = None
    if start is not None:
        out.append((start, len(statements)))
    return out


def vote_ranges(statements, flags):
    """The (ref, start, end) a block votes for, in statement order; flags[0] collects the bits."""
    for st in statements:
        if st[0] == "vote":
            if st[2] == U64:
                flags[0] |= FLAG_OFFSET
            else:
                yield st[1], st[2], st[2] + 1
        elif st[0] == "reject":
            flags[0] |= FLAG_REJECT
        elif st[0] == "range":
            if st[3] < st[2] or st[3] - st[2] >= MAX_RANGE:
                flags[0] |= FLAG_RANGE
            else:
                yield st[1], st[2], st[3]


# ---------------------------------------------------------------- the reference, restated
class RangeMap:
    """range_map.rs: a BTreeMap from range start to (start, end, value)."""

    def __init__(self):
        self.keys = []   # sorted starts
        self.items = {}  # start -> [start, end, v]

    def _insert(self, item):
        assert item[0] not in self.items, "Entry must be vacant"
        bisect.insort(self.keys, item[0])
        self.items[item[0]] = item

    def _remove(self, k):
        self.keys.remove(k)
        del self.items[k]

    def is_empty(self):
        return not self.keys

    def mutate_range(self, start, end, f, clone):
        while True:
            # the item that starts at `start`, or the second half of the one that contains it
            first = None
            j = bisect.bisect_right(self.keys, start)
            if j:
                lb = self.items[self.keys[j - 1]]
                if lb[0] == start:
                    first = lb
                elif lb[1] > start:
                    first = [start, lb[1], clone(lb[2])]
                    lb[1] = start
                    self._insert(first)
            nxt = None
            if first is not None:
                if first[1] == end:
                    overlap = first
                elif first[1] > end:
                    self._insert([end, first[1], clone(first[2])])
                    first[1] = end
                    overlap = self.items[start]
                else:
                    nxt = (first[1], end)
                    overlap = first
            else:
                j = bisect.bisect_left(self.keys, start)
                if j < len(self.keys) and self.keys[j] < end:
                    ub = self.keys[j]
                    nxt = (ub, end)
                    overlap = [start, ub, None]
                else:
                    overlap = [start, end, None]
                self._insert(overlap)
            overlap[2] = f(overlap[0], overlap[1], overlap[2])
            if overlap[2] is None:
                self._remove(overlap[0])
            if nxt is None:
                break
            start, end = nxt


class StakeAggregator:
    def __init__(self):
        self.votes, self.stake = set(), 0

    def add(self, vote, stakes, threshold):
        if vote not in self.votes:
            self.votes.add(vote)
            self.stake += stakes[vote]
        return self.stake >= threshold

    def clone(self):
        c = StakeAggregator()
        c.votes, c.stake = set(self.votes), self.stake
        return c


def _clone(v):
    return None if v is None else v.clone()


class VerbatimAggregator:
    def __init__(self, stakes):
        self.stakes, self.threshold = list(stakes), quorum_threshold(stakes)
        self.pending = {}

    def len(self):
        return len(self.pending)

    def _register(self, ref, start, end, author, acc):
        rm = self.pending.setdefault(ref, RangeMap())

        def f(s, e, agg):
            if agg is not None:
                acc["duplicate"] += e - s
                return agg
            agg = StakeAggregator()
            agg.add(author, self.stakes, self.threshold)
            return agg

        rm.mutate_range(start, end, f, _clone)

    def _vote(self, ref, start, end, author, acc):
        rm = self.pending.get(ref)
        if rm is None:
            acc["unknown"] += end - start
            return

        def f(s, e, agg):
            if agg is None:
                acc["unknown"] += e - s
                return None
            if agg.add(author, self.stakes, self.threshold):
                acc["processed"].extend((ref, l) for l in range(s, e))
                return None
            return agg

        rm.mutate_range(start, end, f, _clone)
        if rm.is_empty():
            del self.pending[ref]

    def process_block(self, blk, register_only=False):
        author, ref, statements = blk
        acc = {"processed": [], "unknown": 0, "duplicate": 0}
        flags = [0]
        for s, e in shared_ranges(statements):
            self._register(ref, s, e, author, acc)
        if not register_only:
            for tgt, s, e in vote_ranges(statements, flags):
                if s != e:  # (an empty range changes nothing but a split)
                    self._vote(tgt, s, e, author, acc)
        return Result(acc["processed"], acc["unknown"], acc["duplicate"], flags[0])


# ---------------------------------------------------------------- the rule per cell
class CellRule:
    def __init__(self, stakes):
        self.stakes, self.threshold = list(stakes), quorum_threshold(stakes)
        self.cells = {}  # ref -> {offset: [voters, stake]}, aggregating cells only
        self.certified = 0

    def len(self):
        return sum(1 for c in self.cells.values() if c)

    def aggregating(self):
        return sum(len(c) for c in self.cells.values())

    def process_block(self, blk, register_only=False):
        author, ref, statements = blk
        processed, unknown, duplicate, flags = [], 0, 0, [0]
        for o, st in enumerate(statements):
            if st[0] != "share":
                continue
            row = self.cells.setdefault(ref, {})
            if o in row:
                duplicate += 1
            else:
                row[o] = [{author}, self.stakes[author]]
        if not register_only:
            for tgt, s, e in vote_ranges(statements, flags):
                row = self.cells.get(tgt)
                if not row:
                    unknown += e - s
                    continue
                top = min(e, max(row) + 1)  # (offsets past the highest aggregating cell are empty)
                unknown += e - max(s, top)
                for o in range(s, top):
                    cell = row.get(o)
                    if cell is None:
                        unknown += 1
                        continue
                    if author not in cell[0]:
                        cell[0].add(author)
                        cell[1] += self.stakes[author]
                    if cell[1] >= self.threshold:
                        processed.append((tgt, o))
                        del row[o]
        self.certified += len(processed)
        return Result(processed, unknown, duplicate, flags[0])
