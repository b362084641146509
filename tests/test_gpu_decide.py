"""GPU: the DAG store (mv_dag_reserve, mv_dag_prune, mv_dag_stats) and the direct decision rule over
it (mv_decide_leaders, mv_dev_decide_leaders) against tests/commit_model.py's DirectRule, which
tests/test_commit_model.py holds to BaseCommitter::try_direct_decide as the reference writes it.
Every row's eight words and three stakes are compared with the model, never with another device
form, at tag widths 64 and 2. Blocks are signed on the GPU and every one is OK for the CPU oracle.
The model's records are the delivered blocks whose whole history was delivered (genesis is seeded
as MV_REF_STORED and has no record)."""
import random

import numpy as np
import pytest

import commit_model as C
import index_model as IM
import mysticeti_amd as M
import replay_model as RM
from mysticeti_amd import blocks as MB
from test_gpu_index import corpus, rand_refs  # noqa: F401  (the same 48 blocks)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def store_engine():
    """A context of its own with the DAG store on (the session engine's connect calls stay as they are)."""
    e = M.Engine(devices=(0,))
    e.dag_reserve(64, 256)
    yield e
    e.close()


@pytest.fixture(params=[64, 2], ids=["tag64", "tag2"])
def tag(request):
    return request.param


def ready(e, tag, pks, stakes, n_auth):
    e.set_committee(pks, np.asarray(stakes, dtype=np.uint64), 0)
    e.set_option("MV_INDEX_TAG_BITS", tag)
    e.index_clear()
    assert e.index_insert_stored(MB.genesis_refs(n_auth)).tolist() == [0] * n_auth


class Dag:
    """Signed blocks layer by layer. A layer is a list of (author, includes) -- a second block of
    an author in one layer equivocates (its time differs)."""

    def __init__(self, engine, n_auth, stakes, distinct):
        self.engine, self.n, self.stakes = engine, n_auth, list(stakes)
        self.seeds = [MB.authority_seed(a) if distinct else bytes(32) for a in range(n_auth)]
        self.pks, _ = MB.committee(engine, n_auth, distinct)
        self.genesis = MB.genesis_refs(n_auth)
        self.bins, self.blocks = [], {}  # in creation order; reference -> (bincode, includes)
        self.rounds = [list(self.genesis)]

    def layer(self, specs):
        rnd = len(self.rounds)
        pres, msgs, seen = [], [], {}
        for a, incs in specs:
            t = rnd * 10**8 + a + 1000 * seen.get(a, 0)
            seen[a] = seen.get(a, 0) + 1
            _, pre = MB.encode(a, rnd, incs, [], [], t, 0, bytes(64), bytes(32))
            pres.append((a, list(incs), t, pre))
            msgs.append(MB._b2(pre))
        seeds = np.frombuffer(b"".join(self.seeds[a] for a, _ in specs), dtype=np.uint8).reshape(-1, 32)
        _, sig = self.engine.ed25519_sign(seeds, np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(-1, 32))
        refs = []
        for (a, incs, t, pre), s in zip(pres, sig):
            s = s.tobytes()
            d = MB._b2(pre + s)
            bn, _ = MB.encode(a, rnd, incs, [], [], t, 0, s, d)
            ref = (a, rnd, d)
            self.bins.append(bn)
            self.blocks[ref] = (bn, incs)
            refs.append(ref)
        self.rounds.append(refs)
        return refs

    def first(self, rnd):
        """The first block of every author at a round, by author."""
        out = {}
        for ref in self.rounds[rnd]:
            out.setdefault(ref[0], ref)
        return [out[a] for a in sorted(out)]

    def full(self, omit=None):
        """A layer where every author includes the first block of every author of the round before;
        omit: {author: authorities it leaves out}."""
        prev = self.first(len(self.rounds) - 1)
        omit = omit or {}
        return self.layer([(a, [r for r in prev if r[0] not in omit.get(a, ())]) for a in range(self.n)])

    def check_oracle(self):
        verdicts = RM.oracle_verdicts(self.pks, np.asarray(self.stakes, dtype=np.uint64), 0)
        assert IM.run_verdicts(verdicts, self.bins) == [0] * len(self.bins)


def stored(blocks, genesis, delivered):
    """The delivered references whose whole history was delivered (the least fixed point of add_blocks)."""
    have, left = set(genesis), list(delivered)
    while True:
        now = [r for r in left if all(i in have for i in blocks[r][1])]
        if not now:
            return [r for r in delivered if r in have]
        have.update(now)
        left = [r for r in left if r not in have]


def model_of(stakes, blocks, records):
    d = C.DirectRule(stakes)
    for ref in records:
        d.add(ref, blocks[ref][1])
    return d


def check_rows(got, rule, leaders, what=""):
    want = [rule.decide(a, r) for a, r in leaders]
    assert got.rows.tolist() == [w.words(a, r) for w, (a, r) in zip(want, leaders)], what
    assert got.stakes.tolist() == [list(w.stakes) for w in want], what
    return want


def corpus_blocks(corpus):
    return {IM.own_ref(b): (b, IM.includes(b)) for b in corpus[0]}


ALL48 = [(a, r) for r in range(0, 13) for a in range(4)]


# ---------------------------------------------------------------- 1. the full DAG
def test_full_dag(store_engine, corpus, tag):
    e = store_engine
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    blocks = corpus_blocks(corpus)
    assert e.connect_blocks(corpus[0]).n_connected == 48
    got = e.decide_leaders(ALL48)
    want = check_rows(got, model_of([1] * 4, blocks, list(blocks)), ALL48)
    for (a, r), row, w in zip(ALL48, got.rows, want):
        if 1 <= r <= 10:
            assert int(row[6]) == M.LEADER_COMMIT and IM.words_ref(row[:6]) == IM.own_ref(corpus[0][4 * (r - 1) + a])
            assert w.stakes == (0, 4, 4) and int(row[7]) == 1
        else:
            assert int(row[6]) == M.LEADER_UNDECIDED
    st = e.dag_stats()
    assert (st.records, st.includes, st.lowest_round, st.highest_round) == (48, 192, 1, 12)


# ---------------------------------------------------------------- 2. the same decisions whatever the delivery
def test_same_decisions_whatever_the_delivery(store_engine, corpus, tag):
    e = store_engine
    bins, blocks = corpus[0], corpus_blocks(corpus)
    final = model_of([1] * 4, blocks, list(blocks))
    # one shuffled call
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    order = list(range(48))
    random.Random(2).shuffle(order)
    assert e.connect_blocks([bins[i] for i in order]).n_connected == 48
    check_rows(e.decide_leaders(ALL48), final, ALL48, "shuffled")
    # round by round, a decide call after each: rows only ever go from UNDECIDED to COMMIT
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    before = [M.LEADER_UNDECIDED] * len(ALL48)
    for r in range(12):
        assert e.connect_blocks(bins[4 * r:4 * r + 4]).n_connected == 4
        got = e.decide_leaders(ALL48)
        check_rows(got, model_of([1] * 4, blocks, [IM.own_ref(b) for b in bins[:4 * r + 4]]), ALL48, r)
        for old, new in zip(before, got.status.tolist()):
            assert new == old or (old, new) == (M.LEADER_UNDECIDED, M.LEADER_COMMIT)
        before = got.status.tolist()
    check_rows(e.decide_leaders(ALL48), final, ALL48, "round by round")
    # in reverse: nothing is stored until round 1 arrives, then earlier calls' blocks are released
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    for r in range(11, 0, -1):
        assert e.connect_blocks(bins[4 * r:4 * r + 4]).n_connected == 0
    assert e.decide_leaders(ALL48).status.tolist() == [M.LEADER_UNDECIDED] * len(ALL48) and e.dag_stats().records == 0
    assert e.connect_blocks(bins[0:4]).n_connected == 48
    check_rows(e.decide_leaders(ALL48), final, ALL48, "reverse")


# ---------------------------------------------------------------- 3..6: small committees
def deliver_and_check(e, tag, dag, leaders, what=""):
    ready(e, tag, dag.pks, dag.stakes, dag.n)
    order = list(range(len(dag.bins)))
    random.Random(len(order)).shuffle(order)
    assert e.connect_blocks([dag.bins[i] for i in order]).n_connected == len(order)
    rule = model_of(dag.stakes, dag.blocks, list(dag.blocks))
    got = e.decide_leaders(leaders)
    return got, check_rows(got, rule, leaders, what)


@pytest.fixture(scope="module")
def blame4(engine):
    d = Dag(engine, 4, [1] * 4, distinct=False)
    d.full()
    d.full({0: [3], 1: [3], 2: [3]})  # round 2: three blame (3, 1)
    d.full({0: [2], 1: [2]})          # round 3: two blame (2, 2)
    d.full()
    d.full()
    d.check_oracle()
    return d


@pytest.fixture(scope="module")
def blame7(engine):
    d = Dag(engine, 7, [5, 1, 1, 1, 1, 1, 1], distinct=True)
    d.full()
    d.full({0: [6]})                          # round 2: the heavy one alone blames (6, 1): 5 of 11
    d.full({0: [5], 1: [5], 2: [5], 3: [5]})  # round 3: the heavy one and three others blame (5, 2): 8 > 7
    d.full()
    d.check_oracle()
    return d


def test_blame_at_its_edge(store_engine, blame4, blame7, tag):
    got, want = deliver_and_check(store_engine, tag, blame4, [(3, 1), (2, 2), (0, 1)])
    assert got.status.tolist() == [M.LEADER_SKIP, M.LEADER_UNDECIDED, M.LEADER_COMMIT]
    assert [w.stakes[0] for w in want] == [3, 2, 0]
    got, want = deliver_and_check(store_engine, tag, blame7, [(6, 1), (5, 2), (0, 1)])
    assert got.status.tolist() == [M.LEADER_UNDECIDED, M.LEADER_SKIP, M.LEADER_COMMIT]  # (6, 1): votes 6 of 11, no quorum
    assert [w.stakes[0] for w in want] == [5, 8, 0]


@pytest.fixture(scope="module")
def weak(engine):
    d = Dag(engine, 4, [1] * 4, distinct=False)
    d.full()
    d.full()
    prev = d.first(2)
    older = d.first(1)[3]
    d.layer([(0, prev[:3] + [older])] + [(a, prev) for a in (1, 2, 3)])  # round 3: author 0 links (3, 1), not (3, 2)
    d.full()
    d.check_oracle()
    return d


def test_weak_link(store_engine, weak, tag):
    got, want = deliver_and_check(store_engine, tag, weak, [(3, 2)])
    assert want[0].stakes == (0, 3, 4) and got.status.tolist() == [M.LEADER_COMMIT]  # neither blame nor vote


@pytest.fixture(scope="module")
def quorums(engine):
    d = Dag(engine, 4, [1] * 4, distinct=False)
    d.full()
    d.full({3: [3]})          # round 2: votes for (3, 1) exactly at quorum: 3
    d.full()
    d.full({2: [2], 3: [2]})  # round 4: votes for (2, 3) one below: 2
    d.full()
    d.full({3: [1]})          # round 6: authors 0, 1, 2 vote for (1, 5)
    d.full({3: [0]})          # round 7: author 3 includes the voting blocks of 1, 2, 3: certificates exactly 3
    d.full()
    d.full({3: [0]})          # round 9: authors 0, 1, 2 vote for (0, 8)
    d.full({2: [0], 3: [0]})  # round 10: only 0 and 1 are certificates: one below
    d.check_oracle()
    return d


def test_votes_and_certificates_at_quorum(store_engine, quorums, tag):
    got, want = deliver_and_check(store_engine, tag, quorums, [(3, 1), (2, 3), (1, 5), (0, 8)])
    assert [w.stakes for w in want] == [(1, 3, 4), (2, 2, 0), (1, 3, 3), (1, 3, 2)]
    assert got.status.tolist() == [M.LEADER_COMMIT, M.LEADER_UNDECIDED, M.LEADER_COMMIT, M.LEADER_UNDECIDED]


@pytest.fixture(scope="module")
def equivocation(engine):
    d = Dag(engine, 4, [1] * 4, distinct=False)
    g = d.genesis
    r1 = d.layer([(a, g) for a in range(4)] + [(3, g[1:] + g[:1])])  # (3, 1) twice: B = r1[3], B' = r1[4]
    b, b2 = r1[3], r1[4]
    # round 2: author 0 includes B' before B and supports B' only; the others vote for B
    d.layer([(0, r1[:3] + [b2, b])] + [(a, r1[:4]) for a in (1, 2, 3)])
    d.full()
    # (2, 4) twice, every author votes for each with a block of its own, and certifies each
    p = d.first(3)
    r4 = d.layer([(a, p) for a in range(4)] + [(2, p[::-1])])
    c, c2 = r4[2], r4[4]
    r5 = d.layer([(a, [x for x in r4[:4] if x != c] + [c]) for a in range(4)] +
                 [(a, [x for x in r4[:4] if x != c] + [c2]) for a in range(4)])
    d.layer([(a, r5[:4]) for a in range(4)] + [(a, r5[4:]) for a in range(4)])
    # (1, 7): author 0 votes with two blocks, author 1 with one, 2 and 3 do not: two authors, not three
    d.full()
    r7 = d.first(7)
    d.layer([(0, r7), (0, r7[::-1]), (1, r7)] + [(a, [x for x in r7 if x[0] != 1]) for a in (2, 3)])
    p8 = d.rounds[8]
    d.layer([(a, p8) for a in range(4)])
    # (0, 10) nine times
    p9 = d.first(9)
    d.layer([(0, p9[k % 4:] + p9[:k % 4]) for k in range(9)] + [(a, p9) for a in (1, 2, 3)])
    d.full()
    d.full()
    d.check_oracle()
    return d, (b, b2, c, c2)


def test_equivocation(store_engine, equivocation, tag):
    dag, (b, b2, c, c2) = equivocation
    leaders = [(3, 1), (2, 4), (1, 7), (0, 10)]
    got, want = deliver_and_check(store_engine, tag, dag, leaders)
    assert got.status.tolist() == [M.LEADER_COMMIT, M.LEADER_CONFLICT, M.LEADER_UNDECIDED, M.LEADER_OVERFLOW]
    assert got.ref(0) == b and want[0].stakes == (0, 3, 4) and got.leader_blocks.tolist() == [2, 2, 1, 9]
    assert want[1].stakes == (0, 4, 4) and want[2].stakes == (2, 2, 0) and want[3].stakes == (0, 0, 0)


# ---------------------------------------------------------------- 7. wide blocks
WIDE_LEADERS = [(31, 1), (32, 1), (63, 1), (64, 1), (99, 1)]


@pytest.fixture(scope="module")
def wide(engine):
    """100 authorities; round 2 blocks include 67 of round 1 (author v: v, v + 1, ... in order, so a
    leader's include stands at every position 0..66 over the voters), round 3 blocks all 100."""
    n = 100
    d = Dag(engine, n, [1] * n, distinct=True)
    r1 = d.full()
    specs = []
    for v in range(n):
        incs = [r1[(v + k) % n] for k in range(67)]
        if v == (31 - 66) % n:  # (31, 1) at position 66: put (31, 0) into the first batch, which moves it to 67
            incs.insert(3, d.genesis[31])
        specs.append((v, incs))
    r2 = d.layer(specs)
    d.layer([(a, r2) for a in range(n)])
    r3 = d.first(3)
    d.layer([(v, [r3[(v + k) % n] for k in range(67)]) for v in range(n)])
    d.check_oracle()
    return d


def test_wide_blocks(store_engine, wide, tag):
    inc = {v: wide.blocks[wide.rounds[2][v]][1] for v in range(100)}
    for a, _ in WIDE_LEADERS:
        where = sorted(inc[v].index(wide.rounds[1][a]) for v in range(100) if wide.rounds[1][a] in inc[v])
        assert {0, 63, 64} <= set(where) and (66 in where or 67 in where)
    got, want = deliver_and_check(store_engine, tag, wide, WIDE_LEADERS + [(31, 2), (5, 3)])
    assert got.status.tolist() == [M.LEADER_COMMIT] * 6 + [M.LEADER_UNDECIDED]
    assert [w.stakes for w in want[:5]] == [(33, 67, 100)] * 5


# ---------------------------------------------------------------- 8. rebuild and prune
def test_rebuild_and_prune(corpus, tag):
    bins, blocks = corpus[0], corpus_blocks(corpus)
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(8)
        e.dag_reserve(2, 2)
        ready(e, tag, corpus[1][0], [1] * 4, 4)
        for r in range(12):
            assert e.connect_blocks(bins[4 * r:4 * r + 4]).n_connected == 4
        final = model_of([1] * 4, blocks, list(blocks))
        check_rows(e.decide_leaders(ALL48), final, ALL48, "grown")
        rng, rebuilds = random.Random(8), e.index_stats().rebuilds
        assert rebuilds >= 1
        while e.index_stats().rebuilds == rebuilds:
            e.index_insert(rand_refs(rng, 100), M.REF_WANTED)
        check_rows(e.decide_leaders(ALL48), final, ALL48, "after the rebuild")
        e.dag_prune(5)
        st = e.dag_stats()
        assert (st.records, st.includes, st.lowest_round, st.highest_round) == (32, 128, 5, 12)
        pruned = model_of([1] * 4, blocks, [r for r in blocks if r[1] >= 5])
        want = check_rows(e.decide_leaders(ALL48), pruned, ALL48, "pruned")
        for (a, r), w in zip(ALL48, want):
            assert w.status == (C.COMMIT if 5 <= r <= 10 else C.UNDECIDED)
        e.dag_prune(3)  # nothing comes back
        assert e.dag_stats().records == 32
        e.index_clear()
        st = e.dag_stats()
        assert (st.records, st.includes, st.lowest_round, st.highest_round) == (0, 0, 0, 0)
        assert e.decide_leaders(ALL48).status.tolist() == [M.LEADER_UNDECIDED] * len(ALL48)
        assert e.index_insert_stored(corpus[2]).tolist() == [0] * 4
        assert e.connect_blocks(bins).n_connected == 48
        check_rows(e.decide_leaders(ALL48), final, ALL48, "after the clear")
    finally:
        e.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals(store_engine, corpus, tag):
    e = M.Engine(devices=(0,))
    try:
        with pytest.raises(M.MvError) as no_committee:
            e.connect_blocks(corpus[0][:4])
        with pytest.raises(M.MvError) as err:
            e.decide_leaders([(0, 1)])
        assert err.value.code == no_committee.value.code == M.E_NO_COMMITTEE
        e.set_committee(*corpus[1])
        with pytest.raises(M.MvError) as err:
            e.decide_leaders([(0, 1)])
        assert err.value.code == M.E_INVALID_ARG
        with pytest.raises(M.MvError) as err:
            e.dag_prune(3)
        assert err.value.code == M.E_INVALID_ARG
        st = e.dag_stats()
        assert (st.records, st.includes, st.lowest_round, st.highest_round) == (0, 0, 0, 0)
    finally:
        e.close()
    e = store_engine
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    assert e.connect_blocks(corpus[0]).n_connected == 48
    assert e.decide_leaders([]).rows.shape == (0, 8)
    got = e.decide_leaders([(4, 3), (1 << 40, 3), (0, 3)])
    assert got.rows[:2].tolist() == [[4, 3, 0, 0, 0, 0, M.LEADER_UNDECIDED, 0], [1 << 40, 3, 0, 0, 0, 0, M.LEADER_UNDECIDED, 0]]
    assert got.stakes[:2].tolist() == [[0, 0, 0]] * 2 and int(got.rows[2, 6]) == M.LEADER_COMMIT


# ---------------------------------------------------------------- 10. the device-buffer variant
def test_device_buffer_variant(store_engine, corpus, tag):
    import torch

    e = store_engine
    ready(e, tag, corpus[1][0], [1] * 4, 4)
    assert e.connect_blocks(corpus[0]).n_connected == 48
    host = e.decide_leaders(ALL48)
    dev = torch.device("cuda", 0)
    n = len(ALL48)
    d_lead = torch.from_numpy(np.asarray(ALL48, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_out = torch.full((n + 1, 8), -3, dtype=torch.int64, device=dev)
    d_stakes = torch.full((n + 1, 3), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    e.dev_decide_leaders(0, d_lead, d_out[:n], d_stakes[:n])
    out, stakes = d_out.cpu().numpy(), d_stakes.cpu().numpy()
    assert (out[n:] == -3).all() and (stakes[n:] == -3).all()
    assert np.array_equal(out[:n].view(np.uint64), host.rows) and np.array_equal(stakes[:n].view(np.uint64), host.stakes)
    e.dev_decide_leaders(0, d_lead, d_out[:n], None)
    check_rows(host, model_of([1] * 4, corpus_blocks(corpus), list(corpus_blocks(corpus))), ALL48)
