"""CPU: the cases of tests/wide_committee.py before the GPU sees them. The stakes meet their four
conditions; every block is OK for the CPU oracle; commit_model's DirectRule equals its Verbatim on
every row, and commit_seq_model's CommitRule its VerbatimCommit on the sequence cases; and across the
cases every bitmap word 0..15 holds a bit of a blame, a vote and a certificate bitmap, each once as
the only bit of its row, so that an edit of a case cannot thin them out silently."""
import pytest

import commit_model as C
import commit_seq_model as S
import wide_committee as W
from test_gpu_decide import model_of


@pytest.fixture(scope="module")
def cases():
    signer = W.OracleSigner()
    return {name: make(signer) for name, make in W.CASES.items()}


def test_the_four_stake_conditions():
    p = W.main_plan()
    assert (p.H, p.m, p.k, sum(p.stakes), p.thr) == (142, 11, 2, 2345, 1563)
    assert W.conditions(p, [W.LIGHT_W4, W.LIGHT_W15]) == 12
    assert 128 <= W.LIGHT_W4 < 160 and 480 <= W.LIGHT_W15 < 512
    for n in W.TOP_SEATS:
        q = W.top_plan(n)
        assert len(q.heavy) == 13 and n - 1 not in q.heavy and max(q.heavy) < n
        assert W.conditions(q, [n - 1]) == 12
        print(n, "heavy stake", q.H, "light seats at the edge", q.k, "quorum_thr", q.thr)


def test_every_block_is_ok_for_the_oracle(cases):
    for name, c in cases.items():
        c.dag.check_oracle()
        assert max(len(incs) for _, incs in c.dag.blocks.values()) <= 40, name
        assert len(c.dag.bins) <= 400, name
    assert cases["blame_edge"].dag.seeds[1] != cases["blame_edge"].dag.seeds[2]  # the one case with distinct keys


def rules(c):
    d = model_of(c.dag.stakes, c.dag.blocks, list(c.dag.blocks))
    v = C.Verbatim(c.dag.stakes)
    for ref, (_, incs) in c.dag.blocks.items():
        v.add(ref, incs)
    return d, v


def test_direct_rule_is_try_direct_decide(cases):
    seen = set()
    for name, c in cases.items():
        d, v = rules(c)
        for a, r in c.leaders:
            got = d.decide(a, r)
            try:
                want = v.try_direct_decide(a, r)
            except C.Panic as e:
                assert "More than one" in str(e)
                want = (C.CONFLICT, None)
            if got.status == C.OVERFLOW:  # the library's own status: more leader blocks than a row tells apart
                assert got.found == 9 and want[0] == C.COMMIT, name
            else:
                assert (got.status, got.ref) == want, (name, a, r, got.stakes)
            seen.add(got.status)
    assert seen == {C.UNDECIDED, C.COMMIT, C.SKIP, C.CONFLICT, C.OVERFLOW}


def test_the_rows_read_what_the_cases_say(cases):
    p = W.main_plan()
    H, thr = p.H, p.thr
    everyone = p.stake(W.PRODUCERS)

    def rows(name):
        c = cases[name]
        d, _ = rules(c)
        return [d.decide(a, r) for a, r in c.leaders]

    for w, row in enumerate(rows("one_blame")):
        s = p.stakes[W.WORD_BLAMERS[w]]
        assert (row.status, row.stakes) == (C.COMMIT, (s, everyone - s, everyone))
    for w, row in enumerate(rows("one_vote")):
        s = p.stakes[W.WORD_LEADERS[w]]
        assert (row.status, row.stakes) == (C.SKIP, (everyone - s, s, 0))
    for w, row in enumerate(rows("one_cert")):
        assert (row.status, row.stakes) == (C.UNDECIDED, (2 * H, thr + 1, p.stakes[W.WORD_LEADERS[w]]))
    assert [(r.status, r.stakes[0]) for r in rows("blame_edge")] == [
        (C.UNDECIDED, thr), (C.SKIP, thr + 1), (C.UNDECIDED, thr), (C.SKIP, thr + 1)]
    assert [(r.status, r.stakes[2]) for r in rows("quorum_edge")] == [(C.COMMIT, thr + 1), (C.UNDECIDED, thr)]
    for (certifiers, enough, short), tip in zip(cases["quorum_edge"].notes["sets"], (510, 256)):
        assert tip in enough and tip in short and 511 in certifiers
        assert p.stake(enough) == thr + 1 and p.stake(short[:-1]) == thr and p.stake(short) == thr + 1
    low, high = p.stake(W.LOW), p.stake(W.HIGH)
    assert [(r.status, r.found, r.stakes) for r in rows("equivocation_0")] == [(C.UNDECIDED, 2, (0, low, 0))]
    assert [(r.status, r.found, r.stakes) for r in rows("equivocation_1")] == [(C.COMMIT, 2, (0, low + high, low + high))]
    assert rows("equivocation_1")[0].ref == cases["equivocation_1"].notes["blocks"][1]
    assert [(r.status, r.found) for r in rows("equivocation_2")] == [(C.CONFLICT, 2)]
    assert [(r.status, r.found, r.stakes) for r in rows("overflow")] == [(C.OVERFLOW, 9, (0, 0, 0)), (C.SKIP, 9, (12 * H, 0, 0))]
    for n in W.TOP_SEATS:
        q = W.top_plan(n)
        assert [(r.status, r.stakes[0]) for r in rows(f"top_blame_{n}")] == [(C.SKIP, q.thr + 1), (C.UNDECIDED, q.thr)]
        assert n - 1 in cases[f"top_blame_{n}"].notes["blamers"][0] and n - 1 not in cases[f"top_blame_{n}"].notes["blamers"][1]
        assert [(r.status, r.stakes[2]) for r in rows(f"top_vote_{n}")] == [(C.COMMIT, q.thr + 1)]
        certifiers, enough, short = cases[f"top_vote_{n}"].notes["sets"][0]
        assert n - 1 in enough and n - 1 in certifiers and n - 1 not in short and q.stake(short[:-1]) == q.thr


@pytest.mark.parametrize("name", ["sequence_linked", "sequence_unlinked"])
def test_commit_rule_is_try_commit(cases, name):
    c = cases[name]
    v, d = S.VerbatimCommit(c.dag.stakes), S.CommitRule(c.dag.stakes)
    for ref, (_, incs) in c.dag.blocks.items():
        v.add(ref, incs)
        d.add(ref, incs)
    rows, sequence = v.try_commit(c.notes["committers"], c.notes["elect"])
    assert [(a, r) for _, _, a, r, _ in rows] == c.leaders and len(c.leaders) == 48
    got, n_seq = d.commit(c.leaders)
    for (st, ref, a, r, direct), g in zip(rows, got):
        assert (g.status, g.ref) == (st, ref), ((a, r), g.info())
        if st in (C.COMMIT, C.SKIP):
            assert g.kind == (S.KIND_DIRECT if direct else S.KIND_INDIRECT)
    assert n_seq == len(sequence) == 48
    at = dict(zip(c.leaders, got))
    g = at[(480, 5)]
    assert (g.kind, c.leaders[g.anchor], g.flags, g.row.stakes) == (S.KIND_INDIRECT, (511, 8), 0, (2 * 142, 1564, 142))
    assert g.status == (C.COMMIT if name == "sequence_linked" else C.SKIP)
    assert all(f.kind == S.KIND_DIRECT and f.status == (C.SKIP if x[0] == 1 else C.COMMIT) for x, f in at.items() if x != (480, 5))


def test_every_word_of_every_bitmap(cases):
    """Per kind of bitmap: the words that hold a bit in some row, and the words that hold the only bit of a row."""
    some = {k: set() for k in ("blame", "vote", "cert")}
    only = {k: set() for k in ("blame", "vote", "cert")}
    for name, c in cases.items():
        d, _ = rules(c)
        for a, r in c.leaders:
            blame, votes, certs = W.bitmaps(c.plan, c.dag.blocks, a, r)
            row = d.decide(a, r)
            assert row.stakes[0] == c.plan.stake(blame), name
            if row.found == 1:
                assert row.stakes[1:] == (c.plan.stake(votes[0]), c.plan.stake(certs[0])), name
            for kind, sets in (("blame", [blame]), ("vote", votes), ("cert", certs)):
                for seats in sets:
                    some[kind] |= W.words_of(seats)
                    if len(seats) == 1:
                        only[kind] |= W.words_of(seats)
    for kind in some:
        assert some[kind] == set(range(16)), kind
        assert only[kind] == set(range(16)), kind
