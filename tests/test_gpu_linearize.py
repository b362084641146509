"""GPU: mv_linearize / mv_dev_linearize / mv_linearize_mark / mv_linearize_stats -- the committed leaders'
sub-DAGs over the DAG store -- against tests/linearize_model.py's LevelRule, which
tests/test_linearize_model.py holds to collect_sub_dag as the reference writes it. Every sub row, every
block row and the stats (marks, last_height) are compared with the model after every call, at tag
widths 64 and 2. DAGs are built, signed and delivered as tests/test_gpu_decide.py does; the model's
records are the blocks the store holds (genesis is seeded as MV_REF_STORED and has no record)."""
import random

import numpy as np
import pytest

import linearize_model as L
import mysticeti_amd as M
from test_gpu_commit import valid_random_dag
from test_gpu_decide import Dag, ready, store_engine, tag, wide  # noqa: F401
from test_gpu_index import rand_refs

pytestmark = pytest.mark.gpu


def refs_of(rows):
    return [(int(r[0]), int(r[1]), np.ascontiguousarray(r[2:]).astype("<u8").tobytes()) for r in rows]


def records_of(dag, floor=1):
    return {ref: list(incs) for ref, (_, incs) in dag.blocks.items() if ref[1] >= floor}


def deliver(e, tag, dag, bins=None):
    ready(e, tag, dag.pks, dag.stakes, dag.n)
    bins = list(dag.bins if bins is None else bins)
    random.Random(len(bins)).shuffle(bins)
    assert e.connect_blocks(bins).n_connected == len(bins)
    st = e.linearize_stats()
    assert (st.marked, st.last_height) == (0, 0)  # mv_index_clear emptied them


def check(e, model, leaders, cap=1 << 12, what=""):
    """One call against the model: rows, blocks, marks and height."""
    got = e.linearize(leaders, cap)
    blocks, sub = model.linearize(leaders, cap)
    assert got.sub.tolist() == sub, what
    assert got.n_rows == len(blocks) and refs_of(got.blocks) == blocks, what
    st = e.linearize_stats()
    assert (st.marked, st.last_height) == (len(model.marked), model.last_height), what
    return got


def first_of(dag, rnd, a=0):
    return dag.first(rnd)[a]


# ---------------------------------------------------------------- fixtures: signed DAGs
@pytest.fixture(scope="module")
def deep(engine):
    """4 seats, 17 full rounds: a block r rounds below a leader stands r includes deep."""
    d = Dag(engine, 4, [1] * 4, distinct=False)
    for _ in range(17):
        d.full()
    return d


@pytest.fixture(scope="module")
def shapes(engine):
    """3 seats, hand-built (every block includes the whole round before, a quorum):
    round 2: the three blocks list round 1 in different orders; C2 carries a duplicate
    round 3: L3 = [A2, B2, C2] -- C2 is popped first, so round 1 hangs below C2 in C2's order
    round 4: A4 equivocates; L4b has a weak link to B1 in front
    round 5: L5 includes both A4 blocks; W5 carries 260 copies of A4 before the rest (j > 255)"""
    d = Dag(engine, 3, [1] * 3, distinct=True)
    a1, b1, c1 = d.full()
    a2, b2, c2 = d.layer([(0, [a1, b1, c1]), (1, [c1, a1, b1]), (2, [b1, c1, b1, a1])])
    a3, b3, c3 = d.layer([(0, [a2, b2, c2]), (1, [c2, b2, a2]), (2, [b2, a2, c2])])
    a4, a4x, b4, c4 = d.layer([(0, [a3, b3, c3]), (0, [c3, b3, a3]), (1, [b1, a3, b3, c3]), (2, [a3, b3, c3])])
    d.layer([(0, [a4, a4x, b4, c4]), (1, [a4] * 260 + [c4, b4, a4x]), (2, [a4, b4, c4])])
    return d


# ---------------------------------------------------------------- 1. one leader per call, all in one call
def test_full_dag_per_call_and_in_one(store_engine, deep, tag):
    e, bins = store_engine, deep.bins[:24]
    records = {r: i for r, i in records_of(deep).items() if r[1] <= 6}
    leaders = [first_of(deep, r, r % 4) for r in range(1, 7)]
    deliver(e, tag, deep, bins)
    m = L.LevelRule(records)
    per_call = [check(e, m, [x], what=f"leader {x[:2]}") for x in leaders]
    assert all(g.status.tolist() == [M.LINEAR_OK] for g in per_call)
    assert any(r[1] == 0 for r in refs_of(per_call[0].blocks))  # seeded genesis: leaves, put out and marked
    deliver(e, tag, deep, bins)
    one = check(e, L.LevelRule(records), leaders, what="in one call")
    assert one.status.tolist() == [M.LINEAR_OK] * 6 and one.sub[:, 3].tolist() == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(one.blocks, np.concatenate([g.blocks for g in per_call]))
    assert one.sub[:, 2].tolist() == [g.n_rows for g in per_call]
    assert e.linearize([]).sub.shape == (0, 4)  # n = 0 does nothing
    assert e.linearize_stats().last_height == 6


# ---------------------------------------------------------------- 2. pop order, duplicates, weak links, equivocation, j > 255
def test_pop_order_is_not_include_order(store_engine, shapes, tag):
    e, d = store_engine, shapes
    deliver(e, tag, d)
    (a1, b1, c1), (a2, b2, c2), l3 = d.rounds[1], d.rounds[2], d.rounds[3][0]
    got = check(e, L.LevelRule(records_of(d)), [l3])
    out = refs_of(got.blocks)
    # C2 is pushed last and popped first: round 1 is C2's list [b1, c1, b1, a1], last pushed first,
    # the duplicate b1 at its lower number -- not A2's [a1, b1, c1], which a breadth-first order gives
    assert [r for r in out if r[1] == 1] == [a1, c1, b1]
    assert [r for r in out if r[1] == 2] == [c2, b2, a2] and out[-1] == l3


def test_weak_link_equivocation_and_wide_include_numbers(store_engine, shapes, tag):
    e, d = store_engine, shapes
    deliver(e, tag, d)
    m = L.LevelRule(records_of(d))
    b4 = d.rounds[4][2]
    got = check(e, m, [b4], what="weak link")
    out, b1 = refs_of(got.blocks), d.rounds[1][1]
    # b1 hangs below the leader itself (include 0), before any round-2 block reaches it
    assert d.blocks[b4][1][0] == b1 and [r for r in out if r[1] == 1][-1] == b1
    l5, w5 = d.rounds[5][0], d.rounds[5][1]
    got = check(e, m, [l5, w5], what="equivocation, then include numbers above 255")
    assert got.status.tolist() == [M.LINEAR_OK] * 2
    assert {d.rounds[4][0], d.rounds[4][1]} <= set(refs_of(got.blocks))  # both blocks of the equivocator
    deliver(e, tag, d)
    got = check(e, L.LevelRule(records_of(d)), [w5], what="include numbers above 255")
    assert [r for r in refs_of(got.blocks) if r[1] == 4] == [d.rounds[4][1], d.rounds[4][2], d.rounds[4][3], d.rounds[4][0]]


def test_wide_round(store_engine, wide, tag):
    """100 seats, 67 and 100 includes per block: past the 64-lane batch."""
    e = store_engine
    deliver(e, tag, wide)
    got = check(e, L.LevelRule(records_of(wide)), [wide.rounds[4][5], wide.rounds[4][6]], what="wide")
    assert got.status.tolist() == [M.LINEAR_OK] * 2 and got.n_rows > 300


# ---------------------------------------------------------------- 3. the rows that are not OK
def test_incomplete_committed_overflow(store_engine, deep, tag):
    e = store_engine
    l3, l4, l5, l16, l17 = (first_of(deep, r) for r in (3, 4, 5, 16, 17))
    bogus = (1, 4, bytes(range(32)))
    records = records_of(deep)
    for name, leaders, status, cap in [
        ("no entry", [l3, bogus, l4], M.LINEAR_INCOMPLETE, 1 << 12),
        ("already marked", [l3, l4, l3, l5], M.LINEAR_COMMITTED, 1 << 12),
        ("reached by an earlier leader of the call", [l4, l3, l5], M.LINEAR_COMMITTED, 1 << 12),
        ("cap", [l3, l4, l5], M.LINEAR_OVERFLOW, 4 + 4 * 3 + 4 - 1),
        ("depth", [l17, l3, l4], M.LINEAR_OVERFLOW, 1 << 12),  # genesis stands 17 includes below l17
    ]:
        deliver(e, tag, deep)
        m = L.LevelRule(records)
        got = check(e, m, leaders, cap, what=name)
        at = got.status.tolist().index(status)
        assert got.status.tolist() == [M.LINEAR_OK] * at + [status] + [M.LINEAR_STOPPED] * (len(leaders) - at - 1), name
        assert e.linearize_stats().last_height == at, name
        check(e, m, leaders[at + 1:], what=name + ": the rows behind, in a call of their own")
    deliver(e, tag, deep)
    got = check(e, L.LevelRule(records), [l16], what="a path exactly as deep as the key")
    assert got.status.tolist() == [M.LINEAR_OK] and got.n_rows == 4 * 16 + 1


def test_missing_record_above_round_0(deep, tag):
    e = M.Engine(devices=(0,))
    try:
        e.dag_reserve(128, 512)
        deliver(e, tag, deep)
        e.dag_prune(2)
        m = L.LevelRule(records_of(deep, floor=2))
        got = check(e, m, [first_of(deep, 2), first_of(deep, 3)], what="pruned below the leader")
        assert got.status.tolist() == [M.LINEAR_INCOMPLETE, M.LINEAR_STOPPED]
        got = check(e, m, [first_of(deep, 1)], what="the leader has no record")
        assert got.status.tolist() == [M.LINEAR_INCOMPLETE]
        # the caller linearizes the pruned part itself and reports it; the marked blocks are passed over
        done = [r for r in deep.blocks if r[1] <= 1] + list(deep.genesis)
        e.linearize_mark(done, 3)
        m.mark(done, 3)
        got = check(e, m, [first_of(deep, 2), first_of(deep, 3)], what="after the report")
        assert got.status.tolist() == [M.LINEAR_OK] * 2 and got.sub[:, 3].tolist() == [4, 5]
        assert all(r[1] >= 2 for r in refs_of(got.blocks))
        e.linearize_mark([], 9)
        assert e.linearize_stats().last_height == 9
    finally:
        e.close()


# ---------------------------------------------------------------- 4. marks outlive rebuilds, growth and pruning
def test_marks_across_rebuild_growth_and_prune(deep, tag):
    e = M.Engine(devices=(0,))
    try:
        with pytest.raises(M.MvError) as err:
            e.linearize([first_of(deep, 1)])
        assert err.value.code == M.E_INVALID_ARG  # mv_dag_reserve first
        e.index_reserve(8)
        e.dag_reserve(1, 1)
        ready(e, tag, deep.pks, deep.stakes, deep.n)
        m = L.LevelRule({})
        for r in range(8):  # the store grows from one record, the index is rebuilt on the way
            layer = deep.bins[4 * r:4 * r + 4]
            assert e.connect_blocks(layer).n_connected == 4
            m.records.update({ref: list(deep.blocks[ref][1]) for ref in deep.rounds[r + 1]})
            if r % 2:
                check(e, m, [first_of(deep, r + 1, r % 4)], what=f"grown to round {r + 1}")
        assert e.index_stats().rebuilds >= 1
        rng, rebuilds = random.Random(8), e.index_stats().rebuilds
        while e.index_stats().rebuilds == rebuilds:
            e.index_insert(rand_refs(rng, 100), M.REF_WANTED)
        st = e.linearize_stats()
        assert (st.marked, st.last_height) == (len(m.marked), 4)
        assert e.connect_blocks(deep.bins[32:48]).n_connected == 16
        m.records.update({ref: list(deep.blocks[ref][1]) for rnd in range(9, 13) for ref in deep.rounds[rnd]})
        check(e, m, [first_of(deep, 10, 1)], what="after the forced rebuild")
        e.dag_prune(9)
        m.records = {r: i for r, i in m.records.items() if r[1] >= 9}
        got = check(e, m, [first_of(deep, 12, 2)], what="after the prune")
        assert got.status.tolist() == [M.LINEAR_OK]
        e.index_clear()
        st = e.linearize_stats()
        assert (st.marked, st.last_height) == (0, 0)
    finally:
        e.close()


# ---------------------------------------------------------------- 5. the device-buffer form
def test_device_buffer_variant(store_engine, deep, tag):
    import torch

    e, bins = store_engine, deep.bins[:24]
    leaders = [first_of(deep, r, 1) for r in (2, 4, 6, 4)]
    deliver(e, tag, deep, bins)
    host = e.linearize(leaders, 64)
    assert host.status.tolist() == [M.LINEAR_OK] * 3 + [M.LINEAR_COMMITTED]
    deliver(e, tag, deep, bins)
    dev, n = torch.device("cuda", 0), len(leaders)
    d_lead = torch.from_numpy(M.ref_words(leaders).view(np.int64).copy()).to(dev)
    d_blocks = torch.full((64 + 1, 6), -3, dtype=torch.int64, device=dev)
    d_sub = torch.full((n + 1, 4), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    rows = e.dev_linearize(0, d_lead, d_blocks[:64], d_sub[:n])
    blocks, sub = d_blocks.cpu().numpy(), d_sub.cpu().numpy()
    assert rows == host.n_rows and (blocks[rows:] == -3).all() and (sub[n:] == -3).all()
    assert np.array_equal(blocks[:rows].view(np.uint64), host.blocks) and np.array_equal(sub[:n].view(np.uint64), host.sub)
    assert e.linearize_stats().last_height == 3


# ---------------------------------------------------------------- 6. random DAGs
@pytest.mark.parametrize("chunk", range(5))
def test_random_dags(engine, store_engine, chunk):
    e = store_engine
    for seed in range(100 + 10 * chunk, 110 + 10 * chunk):
        rng = random.Random(seed)
        n_auth = 4 + seed % 3
        d = Dag(engine, n_auth, [1] * n_auth, distinct=False)
        refs = {(a, 0, 0): d.genesis[a] for a in range(n_auth)}
        for rnd, layer in enumerate(valid_random_dag(seed, n_auth, 8), 1):
            made, seen = d.layer([(a, [refs[i] for i in incs]) for a, incs in layer]), {}
            for (a, _), ref in zip(layer, made):
                refs[(a, rnd, seen.get(a, 0))] = ref
                seen[a] = seen.get(a, 0) + 1
        deliver(e, 2 if seed % 2 else 64, d)
        leaders = [rng.choice(layer) for layer in d.rounds[1:] if rng.random() < 0.6]
        marked = [r for r in d.blocks if rng.random() < 0.08] if seed % 3 == 0 else []
        m = L.LevelRule(records_of(d))
        if marked:
            e.linearize_mark(marked, 2)
            m.mark(marked, 2)
        statuses = []
        for part in (leaders[:len(leaders) // 2], leaders[len(leaders) // 2:]):
            statuses += check(e, m, part, what=f"seed {seed}").status.tolist()
        # (the DAGs are complete and 8 rounds deep: a row is OK, or COMMITTED and what stands behind it)
        assert set(statuses) <= {M.LINEAR_OK, M.LINEAR_COMMITTED, M.LINEAR_STOPPED}, seed
