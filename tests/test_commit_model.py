"""CPU: tests/commit_model.py's DirectRule (the header's wording of mv_decide_leaders) held to its
Verbatim (BaseCommitter::try_direct_decide as the reference writes it) at wave length 3, on seeded
random DAGs and on the scenarios of consensus/tests/base_committer_tests.rs restated by shape.

The monotone property, as the header states it: removing records turns COMMIT or SKIP into
UNDECIDED, never UNDECIDED into anything, and never one COMMIT into another. One case is outside
it and is the reference's too: where authors of more than a third of the stake equivocate in the
voting round, a quorum of blame can stand beside a leader block with enough support; the blame test
comes first (base_committer.rs:326-329), so removing the blaming blocks uncovers the COMMIT. The
test allows SKIP -> COMMIT exactly when the full store had such a block (Row.supported)."""
import random

import pytest

import commit_model as C

ROUNDS = 12
COMMITTEES = {4: [1, 1, 1, 1], 7: [5, 1, 1, 1, 1, 1, 1]}


def delivered(seed, n_auth):
    rng = random.Random(seed * 16 + n_auth)
    dag = C.random_dag(rng, n_auth, ROUNDS)
    return dag[:rng.randint(len(dag) // 3, len(dag))], rng  # a prefix of a causal order is causally closed


def verbatim_rows(blocks, stakes, wave_length=3):
    v = C.Verbatim(stakes, wave_length)
    for ref, incs in blocks:
        v.add(ref, incs)
    out = {}
    for a in range(len(stakes)):
        for r in range(ROUNDS + 1):
            try:
                out[(a, r)] = v.try_direct_decide(a, r)
            except C.Panic as e:
                assert "More than one" in str(e)  # the sub-dag of a prefix is whole
                out[(a, r)] = (C.CONFLICT, None)
    return out


def rule_rows(blocks, stakes):
    d = C.DirectRule(stakes)
    for ref, incs in blocks:
        d.add(ref, incs)
    return {(a, r): d.decide(a, r) for a in range(len(stakes)) for r in range(ROUNDS + 1)}


@pytest.fixture(scope="module")
def runs():
    """(blocks, stakes, Verbatim's rows, rng) for 100 seeds at both committees."""
    out = []
    for seed in range(100):
        for n_auth, stakes in COMMITTEES.items():
            blocks, rng = delivered(seed, n_auth)
            out.append((blocks, stakes, verbatim_rows(blocks, stakes), rng))
    return out


def test_the_mix_of_statuses(runs):
    """From Verbatim alone: the DAGs exercise every status."""
    counts = [0] * 5
    for _, _, rows, _ in runs:
        for st, _ in rows.values():
            counts[st] += 1
    total = sum(counts)
    print("rows", total, "UNDECIDED, COMMIT, SKIP, CONFLICT:", counts[:4])
    for st in (C.COMMIT, C.SKIP, C.UNDECIDED):
        assert 10 * counts[st] >= total, (st, counts)
    assert counts[C.CONFLICT] >= 1


def test_direct_rule_is_try_direct_decide(runs):
    for blocks, stakes, want, _ in runs:
        got = rule_rows(blocks, stakes)
        for key, (st, ref) in want.items():
            assert (got[key].status, got[key].ref) == (st, ref), (key, got[key].stakes)


def test_monotone_in_the_records(runs):
    for blocks, stakes, _, rng in runs[::4]:
        full = rule_rows(blocks, stakes)
        kept = [b for b in blocks if rng.random() < 0.8]
        part = rule_rows(kept, stakes)
        for key, before in full.items():
            after = part[key]
            assert after.stakes[0] <= before.stakes[0]
            if after.status == before.status and after.ref == before.ref:
                continue
            if before.status in (C.UNDECIDED, C.COMMIT):
                assert after.status == C.UNDECIDED, (key, before.status, after.status)
            elif before.status == C.SKIP:
                assert after.status == C.UNDECIDED or before.supported, (key, after.status)


def test_wave_length_is_read(runs):
    """Verbatim takes any wave length: at 4 the decision round is r + 3, so it cannot agree everywhere."""
    blocks, stakes, want, _ = runs[0]
    assert verbatim_rows(blocks, stakes, 4) != want


# ---------------------------------------------------------------- consensus/tests/base_committer_tests.rs, by shape
N = 4
STAKES = [1] * N


def leader(rnd, offset=0):  # Committee::elect_leader in test mode (committee.rs:141-142)
    return (rnd + offset) % N


class Dag:
    def __init__(self):
        self.rng = random.Random(7)
        self.blocks = []
        self.last = self.layer([(a, []) for a in range(N)], 0)

    def layer(self, connections, rnd):  # build_dag_layer
        refs = []
        for a, incs in connections:
            ref = (a, rnd, self.rng.randbytes(32))
            self.blocks.append((ref, list(incs)))
            refs.append(ref)
        return refs

    def build(self, start, stop):  # build_dag: full layers up to round `stop`
        refs = self.last if start is None else start
        for r in range(refs[0][1] + 1, stop + 1):
            refs = self.layer([(a, refs) for a in range(N)], r)
        self.last = refs
        return refs

    def both(self, a, r):
        v, d = C.Verbatim(STAKES), C.DirectRule(STAKES)
        for ref, incs in self.blocks:
            v.add(ref, incs)
            d.add(ref, incs)
        want, got = v.try_direct_decide(a, r), d.decide(a, r)
        assert (got.status, got.ref) == want
        return got


def test_direct_commit():
    dag = Dag()
    dag.build(None, 5)
    row = dag.both(leader(3), 3)
    assert row.status == C.COMMIT and row.ref[:2] == (leader(3), 3) and row.stakes == (0, 4, 4)


def test_idempotence():
    dag = Dag()
    dag.build(None, 5)
    first = dag.both(leader(3), 3)
    again = dag.both(leader(3), 3)
    assert (first.status, first.ref) == (again.status, again.ref) == (C.COMMIT, first.ref)
    dag.build(None, 8)
    assert dag.both(leader(3), 3).ref == first.ref
    row = dag.both(leader(6), 6)
    assert row.status == C.COMMIT and row.ref[1] == 6


def test_multiple_direct_commit():
    dag = Dag()
    for n in range(1, 11):
        dag.build(None, 3 * (n + 1) - 1)
        row = dag.both(leader(3 * n), 3 * n)
        assert row.status == C.COMMIT and row.ref[:2] == (leader(3 * n), 3 * n)
        assert dag.both(leader(3 * n + 3), 3 * n + 3).status == C.UNDECIDED  # its wave has not ended


def test_no_leader():
    dag = Dag()
    refs = dag.build(None, 2)
    refs = dag.layer([(a, refs) for a in range(N) if a != leader(3)], 3)
    dag.build(refs, 5)
    row = dag.both(leader(3), 3)
    assert row.status == C.SKIP and row.found == 0 and row.stakes == (4, 0, 0)


def test_direct_skip():
    dag = Dag()
    refs = dag.build(None, 3)
    dag.build([x for x in refs if x[0] != leader(3)], 5)
    row = dag.both(leader(3), 3)
    assert row.status == C.SKIP and row.found == 1 and row.stakes == (4, 0, 0)


def test_undecided():
    dag = Dag()
    refs = dag.build(None, 3)
    without = [x for x in refs if x[0] != leader(3)]
    refs = dag.layer([(0, refs)] + [(a, without) for a in (1, 2)], 4)  # quorum_threshold() - 1 of them blame
    dag.build(refs, 5)
    row = dag.both(leader(3), 3)
    assert row.status == C.UNDECIDED and row.stakes == (2, 1, 0)
