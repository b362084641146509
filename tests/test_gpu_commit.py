"""GPU: mv_commit_leaders / mv_dev_commit_leaders -- the direct rule, the indirect rule and the decided
prefix over the DAG store -- against tests/commit_seq_model.py's CommitRule, which
tests/test_commit_seq_model.py holds to try_indirect_decide and UniversalCommitter::try_commit as the
reference writes them. Every row's eight out words, its four info words and the sequence's length are
compared with the model, never with another device form, at tag widths 64 and 2. DAGs are built,
signed and delivered as tests/test_gpu_decide.py does; the model's records are the blocks the store
holds (genesis is seeded as MV_REF_STORED and has no record)."""
import random

import numpy as np
import pytest

import commit_model as C
import commit_seq_model as S
import mysticeti_amd as M
from test_gpu_decide import Dag, ready, stored, store_engine, tag  # noqa: F401
from test_gpu_index import rand_refs

pytestmark = pytest.mark.gpu


def rule_of(stakes, blocks, records):
    d = S.CommitRule(stakes)
    for ref in records:
        d.add(ref, blocks[ref][1])
    return d


def check(got, rule, leaders, what=""):
    want, n_seq = rule.commit(leaders)
    assert got.rows.tolist() == [w.row.words(a, r) for w, (a, r) in zip(want, leaders)], what
    assert got.info.tolist() == [w.info() for w in want], what
    assert got.n_sequence == n_seq, what
    decided = [(i, w.status) for i, (w, x) in enumerate(zip(want, leaders)) if x[1] > 0][:n_seq]
    assert got.sequence() == decided and all(st in (C.COMMIT, C.SKIP) for _, st in decided), what
    return dict(zip(leaders, want))


def deliver(e, tag, dag, bins=None, shuffle=True, seeded=()):
    ready(e, tag, dag.pks, dag.stakes, dag.n)
    if seeded:
        assert e.index_insert_stored(list(seeded)).tolist() == [0] * len(seeded)
    bins = list(dag.bins if bins is None else bins)
    if shuffle:
        random.Random(len(bins)).shuffle(bins)
    assert e.connect_blocks(bins).n_connected == len(bins)


def rows_of(committers, dag):
    return S.leader_rows(committers, S.elect_test_mode(dag.n), len(dag.rounds) - 1)


# ---------------------------------------------------------------- 1. the hand-built DAGs
def build_hand(engine, layers):
    d = Dag(engine, 4, [1] * 4, distinct=False)
    refs = {(a, 0, 0): d.genesis[a] for a in range(4)}
    for rnd, layer in enumerate(layers, 1):
        made, seen = d.layer([(a, [refs[i] for i in incs]) for a, incs in layer]), {}
        for (a, _), ref in zip(layer, made):
            refs[(a, rnd, seen.get(a, 0))] = ref
            seen[a] = seen.get(a, 0) + 1
    return d, refs


@pytest.fixture(scope="module")
def hands(engine):
    out = {}
    for name, (committers, layers) in S.HAND.items():
        d, refs = build_hand(engine, layers)
        d.check_oracle()
        out[name] = (d, refs, rows_of(committers, d))
    return out


# name -> what the rows in question must read (status, kind, flags), beside the full comparison
EXPECT = {
    "indirect_skip": {(3, 3): (C.SKIP, 2, 0)},
    "indirect_commit": {(3, 3): (C.COMMIT, 2, 0)},
    "anchor_three_up": {(3, 3): (C.COMMIT, 2, 0), (2, 6): (C.SKIP, 1, 0), (3, 7): (C.SKIP, 1, 0)},
    "chain": {(3, 3): (C.COMMIT, 2, 0), (2, 6): (C.COMMIT, 2, 0)},
    "blocked": {(3, 3): (C.UNDECIDED, 0, 2), (2, 6): (C.UNDECIDED, 0, 0)},
    "weak_link": {(3, 3): (C.SKIP, 2, 0)},
    "round_0": {(1, 0): (C.UNDECIDED, 0, 0)},
    "two_leaders": {(3, 3): (C.COMMIT, 2, 0), (0, 3): (C.COMMIT, 1, 0)},
    "overflow": {(2, 6): (C.OVERFLOW, 1, 0), (3, 3): (C.UNDECIDED, 0, 2)},
}


@pytest.mark.parametrize("name", list(S.HAND))
def test_hand_built(store_engine, hands, tag, name):
    dag, refs, leaders = hands[name]
    deliver(store_engine, tag, dag)
    got = store_engine.commit_leaders(leaders)
    want = check(got, rule_of(dag.stakes, dag.blocks, list(dag.blocks)), leaders, name)
    for key, (status, kind, flags) in EXPECT[name].items():
        i = leaders.index(key)
        assert (int(got.status[i]), int(got.kind[i]), int(got.flags[i])) == (status, kind, flags), (name, key)
    if name == "chain":
        assert leaders[want[(3, 3)].anchor] == (2, 6) and leaders[want[(2, 6)].anchor] == (1, 9)
    if name == "round_0":
        assert got.n_sequence == len(leaders) - 1
    if name == "weak_link":
        assert refs[(0, 5, 0)] in dag.blocks[refs[(3, 7, 0)]][1] and want[(3, 3)].reach == 3


# ---------------------------------------------------------------- 2. a random DAG, whatever the delivery
def valid_random_dag(seed, n_auth=7, rounds=14):
    """commit_model.random_dag with every block topped up to a quorum of the round before (a verified
    block has one): (author, round, k) labels as in commit_seq_model.HAND."""
    rng = random.Random(seed)
    dag = C.random_dag(rng, n_auth, rounds, p_shun=0.45, p_keep=0.93, p_shunned=0.3, p_weak=0.25, p_equiv=0.12, p_shuffle=1.0)
    label, seen, layers = {}, {}, [[] for _ in range(rounds)]
    first = {}
    for ref, incs in dag:
        a, r, _ = ref
        label[ref] = (a, r, seen.get((a, r), 0))
        seen[(a, r)] = seen.get((a, r), 0) + 1
        first.setdefault((a, r), label[ref])
        if r == 0:
            continue
        incs = [label[i] for i in incs]
        prev = {i[0] for i in incs if i[1] == r - 1}
        for b in range(n_auth):
            if 3 * len(prev) > 2 * n_auth:
                break
            if b not in prev:
                prev.add(b)
                incs.append(first[(b, r - 1)])
        layers[r - 1].append((a, incs))
    return layers


@pytest.fixture(scope="module")
def random7(engine):
    d = Dag(engine, 7, [1] * 7, distinct=True)
    refs = {(a, 0, 0): d.genesis[a] for a in range(7)}
    for rnd, layer in enumerate(valid_random_dag(3), 1):
        made, seen = d.layer([(a, [refs[i] for i in incs]) for a, incs in layer]), {}
        for (a, _), ref in zip(layer, made):
            refs[(a, rnd, seen.get(a, 0))] = ref
            seen[a] = seen.get(a, 0) + 1
    d.check_oracle()
    return d


def test_random_dag_whatever_the_delivery(store_engine, random7, tag):
    dag, e = random7, store_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    rule = rule_of(dag.stakes, dag.blocks, list(dag.blocks))
    deliver(e, tag, dag, shuffle=False)
    causal = e.commit_leaders(leaders)
    want = check(causal, rule, leaders, "causal")
    kinds = [(w.status, w.kind) for w in want.values()]
    assert (C.COMMIT, 2) in kinds and (C.SKIP, 2) in kinds and (C.COMMIT, 1) in kinds  # the DAG has work for both rules
    assert any(len(v) > 1 for v in _by_slot(dag).values())  # ... and equivocation
    deliver(e, tag, dag, shuffle=True)
    shuffled = e.commit_leaders(leaders)
    check(shuffled, rule, leaders, "shuffled")
    assert np.array_equal(causal.rows, shuffled.rows) and np.array_equal(causal.info, shuffled.info)


def _by_slot(dag):
    out = {}
    for ref in dag.blocks:
        out.setdefault(ref[:2], []).append(ref)
    return out


# ---------------------------------------------------------------- 3. a block of more than 64 includes on the walk
@pytest.fixture(scope="module")
def wide(engine):
    """70 authorities (a quorum is 47). (1, 1) has 50 votes and 10 certificates (authors 0-9 of round
    3); the anchor (4, 4) includes 65 references, the one certificate among them last."""
    n = 70
    d = Dag(engine, n, [1] * n, distinct=True)
    r1 = d.full()
    r2 = d.layer([(a, [x for x in r1 if x[0] != 1 or a < 50]) for a in range(n)])
    r3 = d.layer([(a, r2 if a < 10 else r2[4:]) for a in range(n)])
    d.layer([(a, r2[:4] + r3[10:] + r3[:1] if a == 4 else r3) for a in range(n)])
    d.full()
    d.full()
    return d


def test_wide_block_on_the_walk(store_engine, wide, tag):
    anchor = wide.first(4)[4]
    incs = wide.blocks[anchor][1]
    assert len(incs) == 65 and incs[64] == wide.first(3)[0]
    leaders = rows_of(S.PIPELINED, wide)
    deliver(store_engine, tag, wide)
    got = store_engine.commit_leaders(leaders)
    want = check(got, rule_of(wide.stakes, wide.blocks, list(wide.blocks)), leaders)
    w = want[(1, 1)]
    assert (w.status, w.kind, leaders[w.anchor], w.reach, w.row.stakes) == (C.COMMIT, 2, (4, 4), 61, (20, 50, 10))


# ---------------------------------------------------------------- 4. an incomplete store
def three_up(votes_only_two):
    r4 = {1: [3], 2: [3]} if votes_only_two else {2: [3]}
    r5 = {} if votes_only_two else {2: [0], 3: [1]}
    return [S._full(1), S._full(2), S._full(3), S._full(4, r4), S._full(5, r5), S._full(6),
            S._full(7, {0: [2], 1: [2], 3: [2]}), S._full(8, {0: [3], 1: [3], 2: [3]}), S._full(9), S._full(10)]


@pytest.fixture(scope="module")
def walks(engine):
    """(3, 3) under the anchor (0, 8), levels 7, 6, 5: an indirect SKIP and an indirect COMMIT."""
    return {k: build_hand(engine, three_up(k == "skip")) for k in ("skip", "commit")}


@pytest.mark.parametrize("which", ["skip", "commit"])
def test_pruned_store(store_engine, walks, tag, which):
    e = store_engine
    dag, refs = walks[which]
    leaders = rows_of(S.PIPELINED, dag)
    at = leaders.index((3, 3))
    deliver(e, tag, dag)
    full = e.commit_leaders(leaders)
    check(full, rule_of(dag.stakes, dag.blocks, list(dag.blocks)), leaders)
    status = C.SKIP if which == "skip" else C.COMMIT
    assert (int(full.status[at]), int(full.kind[at]), int(full.info[at, 3])) == (status, 2, 4)
    e.dag_prune(3)  # the leader's round stays: every record the walk reads survives
    got = e.commit_leaders(leaders)
    check(got, rule_of(dag.stakes, dag.blocks, [r for r in dag.blocks if r[1] >= 3]), leaders, "pruned at 3")
    assert (int(got.status[at]), int(got.flags[at])) == (status, 0)
    e.dag_prune(6)  # inside the walk
    got = e.commit_leaders(leaders)
    check(got, rule_of(dag.stakes, dag.blocks, [r for r in dag.blocks if r[1] >= 6]), leaders, "pruned at 6")
    assert (int(got.status[at]), int(got.kind[at]), int(got.flags[at])) == (C.UNDECIDED, 0, M.COMMIT_INCOMPLETE)
    assert leaders[int(got.info[at, 1])] == (0, 8)


# the seeded reference, and what (3, 3) reads when it was an indirect SKIP / an indirect COMMIT
SEEDED = {
    "a block of the walk": ((1, 6, 0), C.UNDECIDED, C.COMMIT),
    "a decision block": ((2, 5, 0), C.UNDECIDED, C.COMMIT),
    "a voting block": ((2, 4, 0), C.UNDECIDED, C.COMMIT),
    "the leader block": ((3, 3, 0), C.UNDECIDED, C.UNDECIDED),
}


@pytest.mark.parametrize("which", ["skip", "commit"])
@pytest.mark.parametrize("what", list(SEEDED))
def test_seeded_store(store_engine, walks, tag, which, what):
    e = store_engine
    dag, refs = walks[which]
    label, if_skip, if_commit = SEEDED[what]
    seed = refs[label]
    leaders = rows_of(S.PIPELINED, dag)
    at = leaders.index((3, 3))
    deliver(e, tag, dag, bins=[bn for ref, (bn, _) in dag.blocks.items() if ref != seed], seeded=[seed])
    got = e.commit_leaders(leaders)
    check(got, rule_of(dag.stakes, dag.blocks, [r for r in dag.blocks if r != seed]), leaders, what)
    assert int(got.status[at]) == (if_skip if which == "skip" else if_commit)
    assert int(got.flags[at]) == M.COMMIT_INCOMPLETE


# ---------------------------------------------------------------- 5. after an index rebuild
def test_after_a_rebuild(hands, tag):
    dag, _, leaders = hands["chain"]
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(8)
        e.dag_reserve(2, 2)
        deliver(e, tag, dag)
        rule = rule_of(dag.stakes, dag.blocks, list(dag.blocks))
        before = e.commit_leaders(leaders)
        check(before, rule, leaders, "grown")
        rng, rebuilds = random.Random(8), e.index_stats().rebuilds
        assert rebuilds >= 1
        while e.index_stats().rebuilds == rebuilds:
            e.index_insert(rand_refs(rng, 100), M.REF_WANTED)
        after = e.commit_leaders(leaders)
        check(after, rule, leaders, "after the rebuild")
        assert np.array_equal(before.rows, after.rows) and np.array_equal(before.info, after.info)
    finally:
        e.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(store_engine, hands, tag):
    dag, _, leaders = hands["indirect_commit"]
    e = M.Engine(devices=(0,))
    try:
        with pytest.raises(M.MvError) as err:
            e.commit_leaders([(0, 1)])
        assert err.value.code == M.E_NO_COMMITTEE
        e.set_committee(dag.pks, np.asarray(dag.stakes, dtype=np.uint64), 0)
        with pytest.raises(M.MvError) as err:
            e.commit_leaders([(0, 1)])
        assert err.value.code == M.E_INVALID_ARG  # no store
    finally:
        e.close()
    e = store_engine
    deliver(e, tag, dag)
    got = e.commit_leaders([])
    assert got.rows.shape == (0, 8) and got.info.shape == (0, 4) and got.n_sequence == 0
    with pytest.raises(M.MvError) as err:
        e.commit_leaders([(1, 1), (3, 3), (2, 2)])
    assert err.value.code == M.E_INVALID_ARG
    check(e.commit_leaders(leaders), rule_of(dag.stakes, dag.blocks, list(dag.blocks)), leaders)  # ... and nothing broke


# ---------------------------------------------------------------- 7. the device-buffer variant
def test_device_buffer_variant(store_engine, hands, tag):
    import torch

    dag, _, leaders = hands["chain"]
    e = store_engine
    deliver(e, tag, dag)
    host = e.commit_leaders(leaders)
    check(host, rule_of(dag.stakes, dag.blocks, list(dag.blocks)), leaders)
    dev = torch.device("cuda", 0)
    n = len(leaders)
    d_lead = torch.from_numpy(np.asarray(leaders, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_out = torch.full((n + 1, 8), -3, dtype=torch.int64, device=dev)
    d_info = torch.full((n + 1, 4), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    n_seq = e.dev_commit_leaders(0, d_lead, d_out[:n], d_info[:n])
    out, info = d_out.cpu().numpy(), d_info.cpu().numpy()
    assert (out[n:] == -3).all() and (info[n:] == -3).all() and n_seq == host.n_sequence
    assert np.array_equal(out[:n].view(np.uint64), host.rows) and np.array_equal(info[:n].view(np.uint64), host.info)
    with pytest.raises(M.MvError) as err:
        e.dev_commit_leaders(0, d_lead.flip(0).contiguous(), d_out[:n], d_info[:n])
    assert err.value.code == M.E_INVALID_ARG


# ---------------------------------------------------------------- 8. the call leaves no state behind
def test_decide_leaders_is_untouched(store_engine, hands, tag):
    dag, _, leaders = hands["chain"]
    e = store_engine
    deliver(e, tag, dag)
    before = e.decide_leaders(leaders)
    first = e.commit_leaders(leaders)
    after = e.decide_leaders(leaders)
    again = e.commit_leaders(leaders)
    assert np.array_equal(before.rows, after.rows) and np.array_equal(before.stakes, after.stakes)
    assert np.array_equal(first.rows, again.rows) and np.array_equal(first.info, again.info)
    assert first.n_sequence == again.n_sequence
    d = C.DirectRule(dag.stakes)
    for ref, (_, incs) in dag.blocks.items():
        d.add(ref, incs)
    assert before.rows.tolist() == [d.decide(a, r).words(a, r) for a, r in leaders]
