"""CPU: tests/connect_model.py ThreeState -- the restatement of mv_connect_blocks in
include/mysti_verify.h: the index with MV_REF_STORED on top and the suspend / unlock cascade as a
level-by-level sweep over a store of suspended blocks -- held to index_model.Reference, which keeps
BlockManager's own structures (blocks_pending, block_references_waiting, the sequential cascade
of add_blocks, block_manager.rs:48-136). That the sweep is the cascade is checked here, not
assumed: after every call of the 100 seeded deliveries of tests/test_index_model.py the connected
references are newly_blocks_processed as a set, STORED is the store, HAVE-only and the suspended
store are blocks_pending, the missing references agree, and the row order is causal. Verdicts are
the CPU oracle's. The last test holds the built library's exports to the new calls."""
import ctypes
import random

import pytest

import connect_model as CM
import index_model as IM
from test_index_model import N_AUTH, bad_signature, dag  # noqa: F401  (the fixture, the same 48 blocks)


def both(dag, seed=CM.STORED):
    bins, genesis, verdicts = dag
    return CM.Reference3(N_AUTH, verdicts, genesis), CM.ThreeState(verdicts, genesis, seed)


def step(ref, three, blocks, groups, what):
    stored_before = set(three.stored())
    processed, newly, missing = ref.accept3(blocks, groups)
    got = three.connect(blocks, groups)
    assert [s == IM.KNOWN for s in got.blk_state] == processed, what
    assert len(set(got.missing)) == len(got.missing) and set(got.missing) == missing, what
    assert three.missing_blocks(N_AUTH) == ref.missing_blocks(), what
    refs = [r[0] for r in got.rows]
    assert len(set(refs)) == len(refs) == len(newly) and set(refs) == set(newly), what
    assert three.stored() == ref.store, what
    assert three.have_only() == set(ref.blocks_pending) == {p[0] for p in three.pending}, what
    # the suspended store keeps what blocks_pending keeps: the block's own includes
    for own, incs, blk in three.pending:
        assert incs == IM.includes(ref.blocks_pending[own]) and blk == CM.EARLIER, what
    # causal: every include of a row was stored before the call or stands in an earlier row
    by_ref = {IM.own_ref(b): b for b in blocks}
    by_ref.update(step.bodies)
    done = set(stored_before)
    for r, blk, level in got.rows:
        assert all(i in done for i in IM.includes(by_ref[r])), (what, r[:2])
        done.add(r)
    # levels ascend; within a level earlier calls' blocks come first, then this call's by index
    keys = [(level, blk != CM.EARLIER, blk) for _, blk, level in got.rows]
    assert keys == sorted(keys), what
    for i, s in enumerate(got.blk_state):
        if s == CM.SUSPENDED:
            assert IM.own_ref(blocks[i]) in ref.blocks_pending, what
        elif s == IM.NEW:
            assert IM.own_ref(blocks[i]) in ref.store, what
    assert three.stats() == (len(ref.store), len(ref.blocks_pending),
                             sum(len(IM.includes(b)) for b in ref.blocks_pending.values()), got.levels), what
    return got


@pytest.fixture(autouse=True)
def bodies(dag):
    step.bodies = {IM.own_ref(b): b for b in dag[0]}


@pytest.mark.parametrize("seed", range(100))
def test_random_deliveries(dag, seed):
    """The deliveries of test_index_model.test_random_deliveries, draw for draw."""
    bins = dag[0]
    rng = random.Random(seed)
    ref, three = both(dag)
    order = list(range(len(bins)))
    rng.shuffle(order)
    order = [i for i in order if rng.random() > 0.1]  # withheld blocks
    order += rng.sample(order, k=len(order) // 5)  # duplicates, later
    rng.shuffle(order)
    bad = bad_signature(bins[rng.randrange(len(bins))])
    p, call, suspended, deepest = 0, 0, 0, 0
    while p < len(order):
        m = rng.randint(1, 9)
        blocks = [bins[i] for i in order[p:p + m]]
        if rng.random() < 0.15:
            blocks.insert(rng.randrange(len(blocks) + 1), bad)
        if rng.random() < 0.2:
            blocks.append(blocks[0])  # a duplicate inside the call
        kind = rng.randrange(3)
        groups = None if kind == 0 else [0] * len(blocks) if kind == 1 else sorted(rng.randrange(3) for _ in blocks)
        got = step(ref, three, blocks, groups, (seed, call))
        suspended += got.blk_state.count(CM.SUSPENDED)
        deepest = max(deepest, got.levels)
        p, call = p + m, call + 1
    got = step(ref, three, bins, [0] * len(bins), (seed, "rest"))
    assert three.wanted() == set() and three.pending == [] and len(three.stored()) == len(bins) + N_AUTH
    assert suspended > 0 and max(deepest, got.levels) >= 2  # the deliveries do exercise the cascade


def test_round_two_before_round_one(dag):
    bins = dag[0]
    ref, three = both(dag)
    got = step(ref, three, bins[4:8], [7] * 4, "round 2")
    assert got.blk_state == [CM.SUSPENDED] * 4 and got.rows == [] and got.levels == 0
    got = step(ref, three, bins[0:2], None, "half of round 1")
    assert got.blk_state == [IM.NEW] * 2 and [r[1:] for r in got.rows] == [(0, 0), (1, 0)]
    got = step(ref, three, bins[2:4], None, "the rest of round 1")
    # level 0: this call's two blocks; level 1: round 2, suspended by the first call, in its order
    assert [r[1:] for r in got.rows] == [(0, 0), (1, 0)] + [(CM.EARLIER, 1)] * 4 and got.levels == 2
    assert [r[0] for r in got.rows[2:]] == [IM.own_ref(b) for b in bins[4:8]]
    assert three.pending == [] and three.stats()[0] == 8 + N_AUTH


def test_a_rejected_group_parks_nothing(dag):
    bins = dag[0]
    ref, three = both(dag)
    got = step(ref, three, [bins[4], bad_signature(bins[5]), bins[6]], [9, 9, 9], "rejected group")
    assert got.blk_state == [IM.DROPPED, IM.REJECTED, IM.DROPPED]
    assert three.pending == [] and got.rows == [] and three.stats() == (N_AUTH, 0, 0, 0)


def test_descendants_of_a_withheld_block_never_connect(dag):
    bins = dag[0]
    ref, three = both(dag)
    rest = [b for i, b in enumerate(bins) if i != 2]  # authority 2's block of round 1 never arrives
    got = step(ref, three, rest, None, "all but one")
    assert [r[0] for r in got.rows] == [IM.own_ref(bins[i]) for i in (0, 1, 3)] and got.levels == 1
    assert len(three.pending) == 44 and three.wanted() == {IM.own_ref(bins[2])}
    got = step(ref, three, rest, None, "again")
    assert got.blk_state == [IM.KNOWN] * 47 and got.rows == [] and len(three.pending) == 44


def test_genesis_seeded_as_have_connects_nothing(dag):
    bins, genesis, verdicts = dag
    three = CM.ThreeState(verdicts, genesis, seed=IM.HAVE)
    got = three.connect(bins, None)
    assert got.rows == [] and got.blk_state == [CM.SUSPENDED] * 48 and got.missing == []
    assert three.stats() == (0, 48, 4 * 48, 0)
    # ... until the caller says they are stored: then a sweep alone releases everything
    assert three.insert(genesis, CM.STORED) == [IM.HAVE] * N_AUTH
    got = three.connect()
    assert [(r[1], r[2]) for r in got.rows] == [(CM.EARLIER, i // 4) for i in range(48)]
    assert [r[0] for r in got.rows] == [IM.own_ref(b) for b in bins] and three.stats() == (52, 0, 0, 12)


def test_a_sweep_alone_after_an_insert_of_stored(dag):
    """n = 0: the caller stored a block itself (its own proposal) and raises its reference."""
    bins = dag[0]
    ref, three = both(dag)
    step(ref, three, bins[1:8], None, "rounds 1 and 2 without the first block")
    assert len(three.pending) == 4
    own = IM.own_ref(bins[0])
    assert three.insert([own], CM.STORED) == [IM.WANTED]
    got = three.connect()
    assert [(r[0], r[1], r[2]) for r in got.rows] == [(IM.own_ref(b), CM.EARLIER, 0) for b in bins[4:8]]
    assert got.blk_state == [] and three.pending == [] and three.wanted() == set()
    assert three.connect().rows == []


def test_the_library_exports_the_connect_calls():
    import mysticeti_amd as M

    lib = M.load_library()
    new = ["mv_connect_blocks", "mv_dev_connect_blocks", "mv_pending_reserve", "mv_pending_stats", "mv_index_insert_stored"]
    for name in new:
        assert name in M.EXPORTS and isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    assert (M.REF_STORED, M.ACC_SUSPENDED) == (CM.STORED, CM.SUSPENDED) == (3, 5)
    assert M.ACC_STATE[M.ACC_SUSPENDED] == "SUSPENDED" and M.CONNECT_EARLIER == CM.EARLIER
    for method in ("connect_blocks", "dev_connect_blocks", "pending_reserve", "pending_stats", "index_insert_stored"):
        assert callable(getattr(M.Engine, method)), method
