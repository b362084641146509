"""Helper (not a test): the indirect decision rule and the committed sequence, restated twice in
plain Python on top of tests/commit_model.py, for tests/test_commit_seq_model.py (which holds the
two to each other) and tests/test_gpu_commit.py (which holds mv_commit_leaders to the second).

  VerbatimCommit  commit_model.Verbatim plus BlockStore::linked_to_round (block_store.rs:306-327,
                  with its parents.is_empty() break), BaseCommitter::decide_leader_from_anchor
                  (base_committer.rs:184-224), try_indirect_decide (:294-318) and
                  UniversalCommitter::try_commit (universal_committer.rs:30-90) over a list of
                  committers (round_offset, leader_offset): last_decided and the 'outer break,
                  push_front, the round > 0 filter ahead of the take_while. Where a committer
                  panics on "More than one certified block" the row is kept as CONFLICT, which is
                  not decided and stops an anchor scan as Undecided does, so that the rows below it
                  can still be compared.
  CommitRule      the restatement of include/mysti_verify.h (mv_commit_leaders) over DirectRule's
                  records at wave length 3: the rows in sequence order, last to first.

Nothing here is shared with the library's kernels."""
import commit_model as C
from commit_model import COMMIT, CONFLICT, OVERFLOW, SKIP, UNDECIDED

KIND_NONE, KIND_DIRECT, KIND_INDIRECT = range(3)
FLAG_INCOMPLETE, FLAG_BLOCKED = 1, 2
NO_ROW = (1 << 64) - 1


def elect_test_mode(n_auth):  # Committee::elect_leader in test mode (committee.rs:141-142)
    return lambda rnd, offset: (rnd + offset) % n_auth


class VerbatimCommit(C.Verbatim):
    def highest_round(self):
        return max(self.index, default=0)

    def linked_to_round(self, later_block, earlier_round):  # block_store.rs:306-327
        parents = [later_block]
        for r in reversed(range(earlier_round, later_block[0][1])):
            parents = [b for b in self.get_blocks_by_round(r) if any(b[0] in x[1] for x in parents)]
            if not parents:
                break
        return parents

    def decide_leader_from_anchor(self, anchor, authority, rnd):  # base_committer.rs:184-224
        leader_blocks = self.get_blocks_at_authority_round(authority, rnd)
        offset = rnd % self.wave_length
        wave = (rnd - offset) // self.wave_length
        decision_round = wave * self.wave_length + self.wave_length - 1 + offset
        potential = self.linked_to_round(anchor, decision_round)
        certified = []
        for b in leader_blocks:
            all_votes = {}
            if any(self.is_certificate(p, b, all_votes) for p in potential):
                certified.append(b)
        if len(certified) > 1:
            raise C.Panic("More than one certified block")
        return (COMMIT, certified[0][0]) if certified else (SKIP, None)

    def try_indirect_decide(self, authority, rnd, leaders):  # :294-318; leaders: the rows above
        for st, ref, _, r, _ in leaders:
            if not rnd + self.wave_length <= r:
                continue
            if st == COMMIT:
                return self.decide_leader_from_anchor(self.get_block(ref), authority, rnd)
            if st == SKIP:
                continue
            break  # Undecided (and a row kept as CONFLICT)
        return UNDECIDED, None

    def try_commit(self, committers, elect, last_decided=(0, 0)):  # universal_committer.rs:30-90
        """-> (every row of the deque as (status, ref, authority, round, direct), the decided sequence)."""
        leaders = []
        done = False
        for rnd in reversed(range(last_decided[1], max(self.highest_round() - 2, 0) + 1)):
            for round_offset, leader_offset in reversed(committers):
                if rnd < round_offset or (rnd - round_offset) % self.wave_length:  # elect_leader (:91-102)
                    continue
                authority = elect(rnd, leader_offset)
                if (authority, rnd) == last_decided:
                    done = True
                    break
                try:
                    st, ref = self.try_direct_decide(authority, rnd)
                    direct = st != UNDECIDED
                    if not direct:
                        st, ref = self.try_indirect_decide(authority, rnd, leaders)
                except C.Panic as e:
                    assert "More than one" in str(e)
                    st, ref, direct = CONFLICT, None, False
                leaders.insert(0, (st, ref, authority, rnd, direct))
            if done:
                break
        sequence = []
        for row in (x for x in leaders if x[3] > 0):
            if row[0] not in (COMMIT, SKIP):
                break
            sequence.append(row)
        return leaders, sequence


class Final:
    """One row of mv_commit_leaders: row (a commit_model.Row: the out words) and the info words."""

    def __init__(self, row, kind, anchor=NO_ROW, flags=0, reach=0):
        self.row, self.kind, self.anchor, self.flags, self.reach = row, kind, anchor, flags, reach
        self.status, self.ref = row.status, row.ref

    def info(self):
        return [self.kind, self.anchor, self.flags, self.reach]


class CommitRule(C.DirectRule):
    def commit(self, leaders):
        """leaders: (authority, round) in sequence order -> (list of Final, the sequence's length)."""
        leaders = list(leaders)
        assert all(x[1] <= y[1] for x, y in zip(leaders, leaders[1:]))
        have = {ref: incs for ref, incs in self.records}
        by_round = {}
        for ref, _ in self.records:
            by_round.setdefault(ref[1], []).append(ref)
        lowest = min(by_round, default=None)
        out = [None] * len(leaders)
        for i in reversed(range(len(leaders))):
            a, r = leaders[i]
            direct = self.decide(a, r)
            if direct.status != UNDECIDED:
                out[i] = Final(direct, KIND_DIRECT)
                continue
            anchor, blocked = None, False
            for j in range(i + 1, len(leaders)):
                if leaders[j][1] < r + 3 or out[j].status == SKIP:
                    continue
                if out[j].status == COMMIT:
                    anchor = j
                else:
                    blocked = True
                break
            if anchor is None:
                out[i] = Final(direct, KIND_NONE, flags=FLAG_BLOCKED if blocked else 0)
                continue
            # reach: only includes exactly one round below the including block carry the walk
            top = out[anchor].ref
            reach, incomplete = {top}, lowest is None or r < lowest
            for q in reversed(range(r + 2, top[1])):
                incs = {i_ for x in reach for i_ in have[x] if i_[1] == q}
                incomplete |= any(i_ not in have for i_ in incs)
                reach = {i_ for i_ in incs if i_ in have}
            sup = {ref: next((i_ for i_ in incs if i_[:2] == (a, r)), None) for ref, incs in self.records if ref[1] == r + 1}
            for c in reach:
                for v in have[c]:
                    if v[1] == r + 1:
                        incomplete |= v not in have or (sup[v] is not None and sup[v] not in have)
            leader_blocks = [ref for ref, _ in self.records if ref[:2] == (a, r)]
            certified = []
            for b in leader_blocks:
                for c in reach:
                    voters = {v[0] for v in have[c] if v in have and v[1] == r + 1 and sup[v] == b}
                    if self.stake(voters) > self.threshold:
                        certified.append(b)
                        break
            flags = FLAG_INCOMPLETE if incomplete else 0
            found = len(leader_blocks)
            if found > C.MAX_LEADER_BLOCKS:
                st, ref, kind = OVERFLOW, None, KIND_INDIRECT  # (defensive: the direct rule already ended such a row)
            elif len(certified) == 1:
                st, ref, kind = COMMIT, certified[0], KIND_INDIRECT
            elif len(certified) > 1:
                st, ref, kind = CONFLICT, None, KIND_INDIRECT
            elif incomplete:
                st, ref, kind = UNDECIDED, None, KIND_NONE
            else:
                st, ref, kind = SKIP, None, KIND_INDIRECT
            out[i] = Final(C.Row(st, ref, found, direct.stakes, len(certified)), kind, anchor, flags, len(reach))
        n_seq = 0
        for (a, r), f in zip(leaders, out):
            if r == 0:
                continue
            if f.status not in (COMMIT, SKIP):
                break
            n_seq += 1
        return out, n_seq


def leader_rows(committers, elect, highest_round, wave_length=3, last_decided=(0, 0)):
    """The rows try_commit's deque ends in: ascending round, within a round in committer order."""
    rows = []
    for rnd in range(last_decided[1], max(highest_round - 2, 0) + 1):
        this = []
        for round_offset, leader_offset in committers:
            if rnd >= round_offset and (rnd - round_offset) % wave_length == 0:
                this.append((elect(rnd, leader_offset), rnd))
        if last_decided in this:  # the 'outer break: committers run in reverse, rounds downwards
            this = this[this.index(last_decided) + 1:]
        rows += this
    return rows


ONE = [(0, 0)]
PIPELINED = [(0, 0), (1, 0), (2, 0)]
PIPELINED_TWO = [(ro, lo) for ro in range(3) for lo in range(2)]


# ---------------------------------------------------------------- hand-built DAGs, 4 authorities of equal stake
# A DAG is a list of layers for rounds 1, 2, ...; a layer is a list of (author, includes), an include
# a label (author, round, k): the k-th block of that author at that round (round 0: genesis).
# Every block includes a quorum of the round before, as a verified block must.
def _full(rnd, omit=None, authors=range(4), prev=range(4), extra=None):
    omit, extra = omit or {}, extra or {}
    return [(a, [(b, rnd - 1, 0) for b in prev if b not in omit.get(a, ())] + extra.get(a, [])) for a in authors]


def _undecided_3_3(certs=2):
    """Rounds 1-5 in which (3, 3) has a quorum of votes (0, 1, 3) and `certs` certificates, below quorum."""
    r5 = {2: {2: [0], 3: [1]}, 1: {1: [3], 2: [0], 3: [1]}}[certs]
    return [_full(1), _full(2), _full(3), _full(4, {2: [3]}), _full(5, r5)]


def _undecided_2_6():
    """Rounds 7-8 in which (2, 6) has a quorum of votes (0, 2, 3) and two certificates."""
    return [_full(7, {1: [2]}), _full(8, {1: [0], 3: [2]})]


HAND = {
    # two votes only, blame below quorum, the next leader committed
    "indirect_skip": (PIPELINED, [_full(1), _full(2), _full(3), _full(4, {1: [3], 2: [3]})] + [_full(r) for r in range(5, 9)]),
    # a quorum of votes, certificates below quorum, the anchor (2, 6) reaches one
    "indirect_commit": (PIPELINED, _undecided_3_3() + [_full(r) for r in range(6, 9)]),
    # (2, 6) and (3, 7) are skipped, (0, 8) is the anchor: levels 7, 6, 5
    "anchor_three_up": (PIPELINED, _undecided_3_3() + [_full(6), _full(7, {0: [2], 1: [2], 3: [2]}),
                                                       _full(8, {0: [3], 1: [3], 2: [3]}), _full(9), _full(10)]),
    # (3, 3) hangs on (2, 6), which hangs on (1, 9)
    "chain": (PIPELINED, _undecided_3_3() + [_full(6)] + _undecided_2_6() + [_full(r) for r in range(9, 12)]),
    # (2, 6) stays undecided: the DAG ends at its decision round
    "blocked": (PIPELINED, _undecided_3_3() + [_full(6)] + _undecided_2_6()),
    # the one certificate (0, 5) is an include of the anchor (3, 7) two rounds down and of nothing at round 6
    "weak_link": (PIPELINED, _undecided_3_3(certs=1) + [
        _full(6, authors=(0, 1, 3), prev=(1, 2, 3)), _full(7, prev=(0, 1, 3), extra={3: [(0, 5, 0)]}),
        _full(8), _full(9)]),
    # (1, 0) has two votes and two blames
    "round_0": (PIPELINED_TWO, [_full(1, {2: [1], 3: [1]}), _full(2), _full(3), _full(4)]),
    # (3, 3) goes indirect, (0, 3) direct
    "two_leaders": (PIPELINED_TWO, _undecided_3_3() + [_full(r) for r in range(6, 9)]),
    # (2, 6) nine times: OVERFLOW, which blocks (3, 3)
    "overflow": (PIPELINED, _undecided_3_3() + [
        _full(6, authors=(0, 1, 3)) + [(2, [((b + k) % 4, 5, 0) for b in range(4)]) for k in range(9)],
        _full(7), _full(8)]),
}
