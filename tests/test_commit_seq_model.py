"""CPU: tests/commit_seq_model.py's CommitRule (the header's wording of mv_commit_leaders) held to its
VerbatimCommit (try_indirect_decide, linked_to_round and UniversalCommitter::try_commit as the
reference writes them) on complete stores: seeded random DAGs at three committee sizes with equal and
unequal stakes under three sets of committers, and hand-built DAGs for each path of the rule.
Rows where the reference panics ("More than one certified block") are compared as CONFLICT.

Removing records: a final COMMIT or SKIP may become UNDECIDED; a SKIP never becomes COMMIT and a
COMMIT never becomes SKIP -- except where the full store had a quorum of blame beside a leader block
with enough support (test_commit_model.py's exception: a direct SKIP). Held on random removals from the
seeded DAGs and on every single-record removal from the hand-built walks."""
import random

import pytest

import commit_model as C
import commit_seq_model as S

ROUNDS = 12
COMMITTEES = {"4": [1] * 4, "7": [1] * 7, "10": [1] * 10, "4u": [2, 1, 1, 1], "7u": [5, 1, 1, 1, 1, 1, 1],
              "10u": [3, 3, 1, 1, 1, 1, 1, 1, 1, 1]}
COMMITTERS = [S.ONE, S.PIPELINED, S.PIPELINED_TWO]
# thin votes and few certificates often enough that the indirect rule has work
DAG_ARGS = dict(p_shun=0.45, p_keep=0.93, p_shunned=0.3, p_weak=0.25, p_equiv=0.12, p_shuffle=1.0)
SEEDS = range(12)


def verbatim(blocks, stakes):
    v = S.VerbatimCommit(stakes)
    for ref, incs in blocks:
        v.add(ref, incs)
    return v


def rule(blocks, stakes):
    d = S.CommitRule(stakes)
    for ref, incs in blocks:
        d.add(ref, incs)
    return d


def compare(blocks, stakes, committers, want=None):
    """CommitRule against try_commit; -> (rows of try_commit, the Finals, the rows)."""
    elect = S.elect_test_mode(len(stakes))
    if want is None:
        want = verbatim(blocks, stakes).try_commit(committers, elect)
    rows, sequence = want
    leaders = [(a, r) for _, _, a, r, _ in rows]
    assert leaders == S.leader_rows(committers, elect, max(ref[1] for ref, _ in blocks))
    got, n_seq = rule(blocks, stakes).commit(leaders)
    for (st, ref, a, r, direct), g in zip(rows, got):
        assert (g.status, g.ref) == (st, ref), ((a, r), g.info())
        if st in (C.COMMIT, C.SKIP):
            assert g.kind == (S.KIND_DIRECT if direct else S.KIND_INDIRECT)
    assert n_seq == len(sequence)
    assert [(a, r) for _, _, a, r, _ in sequence] == [x for x in leaders if x[1] > 0][:n_seq]
    return rows, got, leaders


@pytest.fixture(scope="module")
def runs():
    """(blocks, stakes, committers, try_commit's answer, rng) for every seed, committee and set of committers."""
    out = []
    for seed in SEEDS:
        for name, stakes in COMMITTEES.items():
            rng = random.Random(seed * 64 + len(name) * 16 + len(stakes))
            blocks = C.random_dag(rng, len(stakes), ROUNDS, **DAG_ARGS)
            v = verbatim(blocks, stakes)
            for committers in COMMITTERS:
                out.append((blocks, stakes, committers, v.try_commit(committers, S.elect_test_mode(len(stakes))), rng))
    return out


def test_the_mix_of_paths(runs):
    """From VerbatimCommit alone: each path of the rule occurs at least 20 times."""
    counts = dict.fromkeys(["direct commit", "direct skip", "indirect commit", "indirect skip", "blocked"], 0)
    for _, _, _, (rows, _), _ in runs:
        for i, (st, _, _, r, direct) in enumerate(rows):
            if st in (C.COMMIT, C.SKIP):
                counts[("direct " if direct else "indirect ") + ("commit" if st == C.COMMIT else "skip")] += 1
            elif st == C.UNDECIDED:
                above = [x[0] for x in rows[i + 1:] if x[3] >= r + 3 and x[0] != C.SKIP]
                counts["blocked"] += bool(above)  # (a COMMIT there would have been the anchor)
    print(counts)
    assert all(c >= 20 for c in counts.values()), counts


def test_commit_rule_is_try_commit(runs):
    for blocks, stakes, committers, want, _ in runs:
        compare(blocks, stakes, committers, want)


def test_removing_records(runs):
    for blocks, stakes, committers, (rows, _), rng in runs[::2]:
        leaders = [(a, r) for _, _, a, r, _ in rows]
        full, _ = rule(blocks, stakes).commit(leaders)
        part, _ = rule([b for b in blocks if rng.random() < 0.85], stakes).commit(leaders)
        for key, before, after in zip(leaders, full, part):
            assert_only_undecides(key, before, after)


def assert_only_undecides(key, before, after):
    if (after.status, after.ref) == (before.status, before.ref) or after.status not in (C.COMMIT, C.SKIP):
        return
    if before.status not in (C.COMMIT, C.SKIP):
        return  # (a row that hung on an undecided one may be decided once that one is skipped)
    assert before.status == C.SKIP and before.kind == S.KIND_DIRECT and before.row.supported, (
        key, before.status, before.kind, after.status, after.kind)


@pytest.mark.parametrize("name", ["indirect_skip", "indirect_commit", "anchor_three_up", "chain", "weak_link"])
def test_removing_one_record_of_a_walk(name):
    """Every record in turn, so each level of each walk loses each of its records once; the row in
    question must have changed for some of them, and then only to UNDECIDED with the incomplete flag."""
    committers, layers = S.HAND[name]
    blocks, _ = build(layers)
    leaders = S.leader_rows(committers, S.elect_test_mode(4), len(layers))
    full, _ = rule(blocks, [1] * 4).commit(leaders)
    at, changed = leaders.index((3, 3)), 0
    for gone in blocks:
        if gone[0][1] == 0:
            continue
        part, _ = rule([b for b in blocks if b is not gone], [1] * 4).commit(leaders)
        for key, before, after in zip(leaders, full, part):
            assert_only_undecides(key, before, after)
        if part[at].status != full[at].status:
            changed += 1
            assert part[at].status == C.UNDECIDED
            assert part[at].flags & (S.FLAG_INCOMPLETE | S.FLAG_BLOCKED) or part[at].anchor == S.NO_ROW
    assert changed >= 3


# ---------------------------------------------------------------- hand-built DAGs
def build(layers, rng=None):
    """The blocks of a hand-built DAG (commit_seq_model.HAND) with random digests, genesis included."""
    rng = rng or random.Random(5)
    refs = {(a, 0, 0): (a, 0, rng.randbytes(32)) for a in range(4)}
    blocks = [(ref, []) for ref in refs.values()]
    for rnd, layer in enumerate(layers, 1):
        seen = {}
        for a, incs in layer:
            ref = (a, rnd, rng.randbytes(32))
            refs[(a, rnd, seen.get(a, 0))] = ref
            seen[a] = seen.get(a, 0) + 1
            blocks.append((ref, [refs[i] for i in incs]))
    return blocks, refs


def hand(name):
    committers, layers = S.HAND[name]
    blocks, refs = build(layers)
    rows, got, leaders = compare(blocks, [1] * 4, committers)
    return {x: g for x, g in zip(leaders, got)}, leaders, refs, blocks


def test_indirect_skip():
    got, leaders, _, _ = hand("indirect_skip")
    g = got[(3, 3)]
    assert (g.status, g.kind, g.flags, g.reach) == (C.SKIP, S.KIND_INDIRECT, 0, 4) and g.row.stakes == (2, 2, 0)
    assert leaders[g.anchor] == (2, 6)
    assert all(got[x].kind == S.KIND_DIRECT and got[x].status == C.COMMIT for x in leaders if x != (3, 3))


def test_indirect_commit():
    got, leaders, refs, _ = hand("indirect_commit")
    g = got[(3, 3)]
    assert (g.status, g.kind, g.ref, g.reach) == (C.COMMIT, S.KIND_INDIRECT, refs[(3, 3, 0)], 4)
    assert g.row.stakes == (1, 3, 2) and leaders[g.anchor] == (2, 6)


def test_anchor_three_leaders_up():
    got, leaders, refs, _ = hand("anchor_three_up")
    assert [got[x].status for x in [(2, 6), (3, 7), (0, 8)]] == [C.SKIP, C.SKIP, C.COMMIT]
    g = got[(3, 3)]
    assert (g.status, g.kind, g.ref) == (C.COMMIT, S.KIND_INDIRECT, refs[(3, 3, 0)]) and leaders[g.anchor] == (0, 8)


def test_chain_of_indirect_commits():
    got, leaders, refs, _ = hand("chain")
    g6, g3 = got[(2, 6)], got[(3, 3)]
    assert (g6.status, g6.kind, leaders[g6.anchor]) == (C.COMMIT, S.KIND_INDIRECT, (1, 9))
    assert (g3.status, g3.kind, leaders[g3.anchor], g3.ref) == (C.COMMIT, S.KIND_INDIRECT, (2, 6), refs[(3, 3, 0)])


def test_blocked_by_an_undecided_row():
    got, leaders, _, blocks = hand("blocked")
    assert (got[(2, 6)].status, got[(2, 6)].flags) == (C.UNDECIDED, 0)
    g = got[(3, 3)]
    assert (g.status, g.kind, g.flags, g.anchor) == (C.UNDECIDED, S.KIND_NONE, S.FLAG_BLOCKED, S.NO_ROW)
    assert rule(blocks, [1] * 4).commit(leaders)[1] == 2


def test_weak_link_does_not_carry_the_walk():
    got, leaders, refs, blocks = hand("weak_link")
    by_ref = dict(blocks)
    cert, anchor = refs[(0, 5, 0)], refs[(3, 7, 0)]
    assert cert in by_ref[anchor] and not any(cert in by_ref[refs[(a, 6, 0)]] for a in (0, 1, 3))
    d = rule(blocks, [1] * 4).decide(3, 3)
    assert d.status == C.UNDECIDED and d.stakes == (1, 3, 1)  # (0, 5) is its one certificate
    g = got[(3, 3)]
    assert (g.status, g.kind, g.reach) == (C.SKIP, S.KIND_INDIRECT, 3) and leaders[g.anchor] == (3, 7)
    assert got[(2, 6)].status == C.SKIP and got[(2, 6)].kind == S.KIND_DIRECT


def test_round_0_row_does_not_shorten_the_prefix():
    got, leaders, _, blocks = hand("round_0")
    assert leaders[0] == (1, 0) and got[(1, 0)].status == C.UNDECIDED and got[(1, 0)].row.stakes == (2, 2, 0)
    assert rule(blocks, [1] * 4).commit(leaders)[1] == len(leaders) - 1 == 4


def test_two_leaders_in_one_round():
    got, leaders, _, _ = hand("two_leaders")
    assert leaders[leaders.index((3, 3)) + 1] == (0, 3)
    assert (got[(3, 3)].status, got[(3, 3)].kind) == (C.COMMIT, S.KIND_INDIRECT)
    assert (got[(0, 3)].status, got[(0, 3)].kind) == (C.COMMIT, S.KIND_DIRECT)
    assert leaders[got[(3, 3)].anchor] == (2, 6)


def test_overflow_blocks_the_rows_below():
    committers, layers = S.HAND["overflow"]
    blocks, _ = build(layers)
    leaders = S.leader_rows(committers, S.elect_test_mode(4), 8)
    got, n_seq = rule(blocks, [1] * 4).commit(leaders)
    got = dict(zip(leaders, got))
    assert got[(2, 6)].status == C.OVERFLOW and got[(2, 6)].row.found == 9
    assert (got[(3, 3)].status, got[(3, 3)].flags) == (C.UNDECIDED, S.FLAG_BLOCKED) and n_seq == 2
