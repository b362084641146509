"""GPU: mv_connect_blocks -- the accept call, the suspended-block store and the level-by-level sweep
that releases it (include/mysti_verify.h) -- with mv_dev_connect_blocks, mv_pending_reserve,
mv_pending_stats and mv_index_insert_stored, against tests/connect_model.py: ThreeState restates
the header over a dict and a list (and tests/test_connect_model.py holds it to BlockManager's own
structures). Verdicts are the CPU oracle's. After every call the statuses, states, missing
references, every connected row in order, the state of every reference of the DAG and the
store's counts are compared with the model, never with another device form. Both tag widths run,
so that at two bits nearly every probe meets a foreign slot with its own tag."""
import random

import numpy as np
import pytest

import connect_model as CM
import index_model as IM
import mysticeti_amd as M
import replay_model as RM
from mysticeti_amd import blocks as MB
from test_gpu_index import N_AUTH, ROUNDS, S64, bad_signature, corpus, rand_refs  # noqa: F401  (the same 48 blocks)

pytestmark = pytest.mark.gpu

EARLIER = M.CONNECT_EARLIER


@pytest.fixture(params=[64, 2], ids=["tag64", "tag2"])
def eng(request, engine, corpus, opts):
    """The session engine with the committee set, the tag width of the case, an empty index and an
    empty store."""
    engine.set_committee(*corpus[1])
    opts("MV_INDEX_TAG_BITS", request.param)
    engine.index_clear()
    yield engine
    engine.index_clear()


@pytest.fixture(params=[64, 2], ids=["tag64", "tag2"])
def fresh(request, corpus, opts):
    """A context of its own (nothing reserved, nothing grown) at the tag width of the case."""
    e = M.Engine(devices=(0,))
    try:
        e.set_committee(*corpus[1])
        e.set_option("MV_INDEX_TAG_BITS", request.param)
        yield e
    finally:
        e.close()


def all_refs(corpus):
    return list(corpus[2]) + [IM.own_ref(b) for b in corpus[0]]


def check_state(e, three, refs, what=""):
    """The state of every reference, the index's counts, the WANTED list and the store's counts."""
    refs = list(dict.fromkeys(list(refs) + list(three.state)))
    assert e.index_lookup(refs).tolist() == [three.lookup(r) for r in refs], what
    st = e.index_stats()
    assert (st.have, st.wanted) == three.counts(), (what, st.have, st.wanted, three.counts())
    rows, total = e.index_wanted()
    assert total == st.wanted and {IM.words_ref(r) for r in rows} == three.wanted(), what
    ps = e.pending_stats()
    assert (ps.stored, ps.suspended, ps.includes, ps.levels) == three.stats(), (what, vars(ps), three.stats())


def check_call(got, want, what=""):
    assert got.blk_status.tolist() == want.blk_status, (what, got.blk_status.tolist(), want.blk_status)
    assert got.blk_state.tolist() == want.blk_state, (what, got.blk_state.tolist(), want.blk_state)
    assert got.n_missing == want.n_missing and np.array_equal(got.missing, IM.ref_words(want.missing)), what
    assert got.n_connected == want.n_connected, (what, got.n_connected, want.n_connected)
    assert np.array_equal(got.connected, CM.rows_words(want.rows)), (what, got.connected[:, 6:].tolist(), [r[1:] for r in want.rows])


def connect(e, three, corpus, blocks=(), groups=None, what=""):
    got = e.connect_blocks(blocks, groups)
    want = three.connect(blocks, groups)
    check_call(got, want, what)
    check_state(e, three, all_refs(corpus), what)
    return got, want


def model(corpus, e, seed=CM.STORED):
    three = CM.ThreeState(corpus[3], corpus[2], seed)
    if seed == CM.STORED:
        assert e.index_insert_stored(corpus[2]).tolist() == [0] * N_AUTH
    else:
        assert e.index_insert(corpus[2], seed).tolist() == [0] * N_AUTH
    return three


# ---------------------------------------------------------------- 1. the whole DAG in one shuffled call
def test_the_dag_in_one_shuffled_call(eng, corpus):
    bins = corpus[0]
    three = model(corpus, eng)
    order = list(range(48))
    random.Random(1).shuffle(order)
    got, _ = connect(eng, three, corpus, [bins[i] for i in order], [0] * 48, "one call")
    assert got.n_connected == 48 and got.blk_state.tolist() == [M.ACC_NEW] * 48
    for row in got.connected:
        assert int(row[7]) == int(row[1]) - 1 and IM.own_ref(bins[order[int(row[6])]]) == IM.words_ref(row[:6])
    assert eng.pending_stats().levels == ROUNDS
    got, _ = connect(eng, three, corpus, bins, None, "again")
    assert got.blk_state.tolist() == [M.ACC_KNOWN] * 48 and got.n_connected == 0


# ---------------------------------------------------------------- 2. round by round in reverse
def test_round_by_round_in_reverse(eng, corpus):
    bins = corpus[0]
    three = model(corpus, eng)
    for r in range(ROUNDS - 1, 0, -1):
        got, _ = connect(eng, three, corpus, bins[4 * r:4 * r + 4], [r] * 4, f"round {r + 1}")
        assert got.n_connected == 0 and got.blk_state.tolist() == [M.ACC_SUSPENDED] * 4
    assert eng.pending_stats().suspended == 44
    got, _ = connect(eng, three, corpus, bins[0:4], [0] * 4, "round 1")
    assert got.n_connected == 48 and eng.pending_stats().levels == ROUNDS
    assert got.connected[:4, 6].tolist() == [0, 1, 2, 3] and (got.connected[4:, 6] == EARLIER).all()
    assert got.connected[:, 7].tolist() == [k // 4 for k in range(48)]
    # within a level the order the blocks were suspended in: the round's four, by index
    assert [IM.words_ref(r[:6]) for r in got.connected] == [IM.own_ref(b) for b in bins]
    assert eng.pending_stats().suspended == 0


# ---------------------------------------------------------------- 3. random deliveries
@pytest.mark.parametrize("seed", range(20))
def test_random_deliveries(eng, corpus, seed):
    """Withheld blocks, duplicates across and inside calls, a bad signature, the three group kinds."""
    bins = corpus[0]
    rng = random.Random(1000 + seed)
    three = model(corpus, eng)
    order = list(range(48))
    rng.shuffle(order)
    order = [i for i in order if rng.random() > 0.1]
    order += rng.sample(order, k=len(order) // 5)
    rng.shuffle(order)
    bad = bad_signature(bins[rng.randrange(48)])
    p = 0
    while p < len(order):
        m = rng.randint(1, 12)
        blocks = [bins[i] for i in order[p:p + m]]
        if rng.random() < 0.25:
            blocks.insert(rng.randrange(len(blocks) + 1), bad)
        if rng.random() < 0.2:
            blocks.append(blocks[0])
        kind = rng.randrange(3)
        groups = None if kind == 0 else [0] * len(blocks) if kind == 1 else sorted(rng.randrange(3) for _ in blocks)
        connect(eng, three, corpus, blocks, groups, (seed, p))
        p += m
    connect(eng, three, corpus, bins, [0] * 48, (seed, "rest"))
    assert three.pending == [] and len(three.stored()) == 52


# ---------------------------------------------------------------- 4. a block never delivered
def test_a_block_never_delivered(eng, corpus):
    bins = corpus[0]
    three = model(corpus, eng)
    rest = [b for i, b in enumerate(bins) if i != 2]
    got, _ = connect(eng, three, corpus, rest, None, "all but one")
    assert got.n_connected == 3 and got.n_missing == 1
    rows, total = eng.index_wanted()
    assert total == 1 and IM.words_ref(rows[0]) == IM.own_ref(bins[2])
    assert eng.index_lookup([IM.own_ref(b) for b in bins[4:]]).tolist() == [M.REF_HAVE] * 44
    got, _ = connect(eng, three, corpus, rest, None, "again")
    assert got.n_connected == 0 and got.blk_state.tolist() == [M.ACC_KNOWN] * 47
    got, _ = connect(eng, three, corpus, (), None, "a sweep alone")
    assert got.n_connected == 0 and eng.pending_stats().suspended == 44


# ---------------------------------------------------------------- 5. growth under suspension
def test_growth_under_suspension(fresh, corpus):
    """The store holds slots of the table: a rebuild re-resolves them."""
    bins = corpus[0]
    e = fresh
    e.index_reserve(8)
    three = model(corpus, e)
    for r in range(ROUNDS - 1, 0, -1):
        connect(e, three, corpus, bins[4 * r:4 * r + 4], None, f"round {r + 1}")
    assert e.pending_stats().suspended == 44
    rng = random.Random(5)
    rebuilds = e.index_stats().rebuilds
    assert rebuilds >= 1
    while e.index_stats().rebuilds == rebuilds:
        extra = rand_refs(rng, 100)
        assert e.index_insert(extra, M.REF_WANTED).tolist() == three.insert(extra, IM.WANTED)
    check_state(e, three, all_refs(corpus), "after the rebuild")
    got, _ = connect(e, three, corpus, bins[0:4], None, "round 1")
    assert got.n_connected == 48 and e.pending_stats().suspended == 0


# ---------------------------------------------------------------- 6. caps
@pytest.mark.parametrize("cap", [0, 1, 47, 48, 51])
def test_caps(eng, corpus, cap):
    bins = corpus[0]
    three = model(corpus, eng)
    connect(eng, three, corpus, bins[4:], None, "rounds 2..12")
    want = three.connect(bins[0:4], None)
    assert want.n_connected == 48
    out = np.full((cap + 2, 8), S64, dtype=np.uint64)
    got = eng.connect_blocks(bins[0:4], None, cap_connected=cap, connected_out=out)
    w = min(cap, 48)
    assert got.n_connected == 48 and (out[w:] == S64).all()
    assert np.array_equal(out[:w], CM.rows_words(want.rows)[:w])
    check_state(eng, three, all_refs(corpus), cap)  # the states rise in full whatever the cap


# ---------------------------------------------------------------- 7. include counts at the lane edges
@pytest.fixture(scope="module")
def committee70(engine):
    """70 authorities of which the first holds more than two thirds of the stake, so that a block
    that includes its block of the round before passes the threshold clock whatever else it includes."""
    n = 70
    seeds = [MB.authority_seed(a) for a in range(n)]
    pks, _ = MB.committee(engine, n, distinct=True)
    stakes = np.ones(n, dtype=np.uint64)
    stakes[0] = 1000
    return n, seeds, pks, stakes


@pytest.mark.parametrize("k", [1, 63, 64, 65, 67])
def test_include_counts_at_the_lane_edges(engine, committee70, k):
    """A check is a wave per block over its includes, 64 at a time: a block with k includes is
    suspended on its last include only, and released when that include arrives."""
    n, seeds, pks, stakes = committee70
    engine.set_committee(pks, stakes, 0)
    engine.index_clear()
    try:
        bins = MB.build_rounds(engine, 2, n, seeds, n_inc=k, n_vr=0, with_tx=False)
        genesis = MB.genesis_refs(n)
        three = CM.ThreeState(RM.oracle_verdicts(pks, stakes, 0), genesis)
        assert engine.index_insert_stored(genesis).tolist() == [0] * n
        top = bins[n]  # authority 0's block of round 2: its own block of round 1 first, then the others'
        incs = IM.includes(top)
        assert len(incs) == k and len(set(incs)) == k
        by_ref = {IM.own_ref(b): b for b in bins[:n]}
        first = [by_ref[r] for r in incs[:-1]] + [top]
        got, want = engine.connect_blocks(first), three.connect(first)
        check_call(got, want, k)
        assert got.blk_state.tolist() == [M.ACC_NEW] * (k - 1) + [M.ACC_SUSPENDED] and got.n_connected == k - 1
        assert got.n_missing == 1 and IM.words_ref(got.missing[0]) == incs[-1]
        ps = engine.pending_stats()
        assert (ps.stored, ps.suspended, ps.includes, ps.levels) == three.stats() == (n + k - 1, 1, k, min(k - 1, 1))
        got, want = engine.connect_blocks([by_ref[incs[-1]]]), three.connect([by_ref[incs[-1]]])
        check_call(got, want, k)
        assert got.connected[:, 6:].tolist() == [[0, 0], [EARLIER, 1]] and IM.words_ref(got.connected[1, :6]) == IM.own_ref(top)
        refs = genesis + [IM.own_ref(b) for b in bins[:n + 1]]
        assert engine.index_lookup(refs).tolist() == [three.lookup(r) for r in refs]
        assert engine.pending_stats().suspended == 0
    finally:
        engine.index_clear()


# ---------------------------------------------------------------- 7b. levels wider than a workgroup
@pytest.fixture(scope="module")
def wide(engine):
    """Three rounds of 260 authorities (more than a workgroup of 256 records per round), each block
    with its own block of the round before and one other's; authority 0 holds the stake, as above."""
    n = 260
    seeds = [MB.authority_seed(a) for a in range(n)]
    pks, _ = MB.committee(engine, n, distinct=True)
    stakes = np.ones(n, dtype=np.uint64)
    stakes[0] = 4 * n
    bins = MB.build_rounds(engine, 3, n, seeds, n_inc=2, n_vr=0, with_tx=False)
    return (bins, (pks, stakes, 0), MB.genesis_refs(n), RM.oracle_verdicts(pks, stakes, 0)), n


@pytest.fixture
def wide_eng(engine, wide):
    engine.set_committee(*wide[0][1])
    engine.index_clear()
    yield engine
    engine.index_clear()


def wide_model(e, wide):
    corpus, n = wide
    assert e.index_insert_stored(corpus[2]).tolist() == [0] * n
    return CM.ThreeState(corpus[3], corpus[2], CM.STORED)


def test_three_levels_of_more_than_a_workgroup(wide_eng, wide):
    """One shuffled call: level 0 lists 260 rows, and the scans of levels 1 and 2 place theirs, from
    three workgroups of records each, behind the rows so far. Rows, levels and order are the model's."""
    corpus, n = wide
    three = wide_model(wide_eng, wide)
    order = list(range(3 * n))
    random.Random(7).shuffle(order)
    got, _ = connect(wide_eng, three, corpus, [corpus[0][i] for i in order], None, "wide")
    assert got.n_connected == 3 * n and got.connected[:, 7].tolist() == [0] * n + [1] * n + [2] * n
    for lv in range(3):  # within a level: arrival order
        at = got.connected[lv * n:(lv + 1) * n, 6].tolist()
        assert at == sorted(at) and all(order[int(i)] // n == lv for i in at)
    assert wide_eng.pending_stats().levels == 3


def test_one_parent_releases_more_than_a_workgroup(wide_eng, wide):
    """Rounds 2 and 3 wait, shuffled together, for authority 0's blocks of rounds 1 and 2. Its block
    of round 1 releases 259 blocks of round 2 in one level; the 260 of round 3 stay, interleaved
    with them, and the compaction keeps each with its includes: its block of round 2 releases them."""
    corpus, n = wide
    bins = corpus[0]
    three = wide_model(wide_eng, wide)
    late = [i for i in range(n, 3 * n) if i != n]
    random.Random(8).shuffle(late)
    got, _ = connect(wide_eng, three, corpus, bins[1:n] + [bins[i] for i in late], None, "waiting")
    assert got.n_connected == n - 1 and wide_eng.pending_stats().suspended == 2 * n - 1
    got, _ = connect(wide_eng, three, corpus, [bins[0]], None, "round 1")
    assert got.connected[:, 7].tolist() == [0] + [1] * (n - 1) and wide_eng.pending_stats().suspended == n
    assert all(int(r[1]) == 2 and int(r[6]) == EARLIER for r in got.connected[1:])
    got, _ = connect(wide_eng, three, corpus, [bins[n]], None, "round 2")
    assert got.connected[:, 7].tolist() == [0] + [1] * n and wide_eng.pending_stats().suspended == 0
    want = [IM.own_ref(bins[i]) for i in late if i >= 2 * n]  # in arrival order
    assert [IM.words_ref(r[:6]) for r in got.connected[1:]] == want


def test_groups_across_a_workgroup_edge(wide_eng, wide):
    """257 blocks in groups of three: the group numbers of the second workgroup's block stand behind
    the first workgroup's heads. A bad signature at block 256 drops block 255, its group's other block."""
    corpus, _ = wide
    three = wide_model(wide_eng, wide)
    blocks = list(corpus[0][:257])
    blocks[256] = bad_signature(blocks[256])
    got, _ = connect(wide_eng, three, corpus, blocks, [i // 3 for i in range(257)], "grouped")
    assert got.blk_state.tolist() == [M.ACC_NEW] * 255 + [M.ACC_DROPPED, M.ACC_REJECTED]


# ---------------------------------------------------------------- 8. the device call
def dev_connect(e, blocks, groups, cap, cap_rows, pad=16):
    """mv_dev_connect_blocks on a device buffer that ends `pad` bytes after the last block."""
    import torch

    dev = torch.device("cuda", 0)
    buf, offs, lens = MB.pack(blocks)
    total = int(lens.sum())
    d_buf = torch.zeros(total + pad, dtype=torch.uint8, device=dev)
    d_buf[:total] = torch.from_numpy(buf[:total].copy()).to(dev)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)
    n = len(blocks)
    d_st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=dev)
    d_state = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=dev)
    d_miss = torch.full((cap + 2, 6), -3, dtype=torch.int64, device=dev)
    d_rows = torch.full((cap_rows + 2, 8), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    nm, nc = e.dev_connect_blocks(0, d_buf, total, t64(offs), t64(lens), t64(groups) if groups is not None else None,
                                  d_st[:n], d_state[:n], d_miss[:cap], d_rows[:cap_rows])
    st, state, miss, rows = d_st.cpu().numpy(), d_state.cpu().numpy(), d_miss.cpu().numpy(), d_rows.cpu().numpy()
    w, wc = min(nm, cap), min(nc, cap_rows)
    assert (st[n:] == 0xAB).all() and (state[n:] == 0xAB).all() and (miss[w:] == -3).all() and (rows[wc:] == -3).all()
    return M.Connected(st[:n], state[:n], miss[:w].view(np.uint64), nm, rows[:wc].view(np.uint64), nc)


def test_device_call(fresh, corpus):
    """16 bytes of padding behind a 55-byte block that comes last; a store reserved too small is
    MV_E_INDEX_FULL with index and store as they were; then a call that fits."""
    bins = corpus[0]
    e = fresh
    e.index_reserve(64)
    three = model(corpus, e)
    blocks = [bins[4], bins[5], bins[0], bins[0][:55]]  # two of round 2, one of round 1, a short block
    probe = all_refs(corpus)
    before = e.index_lookup(probe).tolist()
    for blocks_cap, inc_cap in ((0, 0), (2, 8), (3, 8)):  # 3 blocks with 12 includes may join the store
        if blocks_cap:
            e.pending_reserve(blocks_cap, inc_cap)
        with pytest.raises(M.MvError) as err:
            dev_connect(e, blocks, [0, 0, 0, 1], cap=16, cap_rows=8)
        assert err.value.code == M.E_INDEX_FULL
        assert e.index_lookup(probe).tolist() == before
        check_state(e, three, probe, (blocks_cap, inc_cap))
    e.pending_reserve(3, 12)
    got = dev_connect(e, blocks, [0, 0, 0, 1], cap=16, cap_rows=8)
    want = three.connect(blocks, [0, 0, 0, 1])
    check_call(got, want, "fits")
    assert got.blk_state.tolist() == [M.ACC_SUSPENDED, M.ACC_SUSPENDED, M.ACC_NEW, M.ACC_REJECTED]
    assert got.n_missing == 3 and got.connected[:, 6:].tolist() == [[2, 0]]
    check_state(e, three, probe, "fits")
    # the rest of round 1, with room for it beside the two blocks the store holds
    e.pending_reserve(5, 20)
    got = dev_connect(e, bins[1:4], None, cap=16, cap_rows=1)
    want = three.connect(bins[1:4], None)
    assert got.n_connected == 5 and np.array_equal(got.connected, CM.rows_words(want.rows)[:1])
    check_state(e, three, probe, "round 1")


# ---------------------------------------------------------------- 9. batch size
def test_batch_size_call(engine, corpus):
    """4,200 blocks in one call (the shape of test_gpu_index.test_batch_size_call): 100 KNOWN copies
    of a stored block, one bad signature, and authority 2's block of round 1 withheld, so that
    only two blocks connect and 44 are parked. The others take the walk and one combined equation."""
    bins = corpus[0]
    engine.set_committee(*corpus[1])
    engine.index_clear()
    try:
        three = model(corpus, engine)
        connect(engine, three, corpus, [bins[0]], None, "first")
        pool = [b for i, b in enumerate(bins) if i not in (0, 2)]
        blocks = [bins[0] if i % 42 == 0 else pool[i % len(pool)] for i in range(4200)]
        blocks[2345] = bad_signature(blocks[2345])
        groups = [i // 100 for i in range(4200)]
        before = engine.batch_counters()[0]
        got, want = connect(engine, three, corpus, blocks, groups, "batch")
        assert engine.batch_counters()[0] == before + 1 and 4200 - 100 >= M.BATCH_MIN
        counts = np.bincount(got.blk_state, minlength=6).tolist()
        print(f"batch: states {counts}, rows {got.n_connected}, stats {vars(engine.pending_stats())}")
        assert counts[M.ACC_KNOWN] == 100 and counts[M.ACC_REJECTED] == 1 and counts[M.ACC_DROPPED] > 0
        assert counts[M.ACC_NEW] == 2 and counts[M.ACC_SUSPENDED] == 44 and got.n_connected == 2
        got, _ = connect(engine, three, corpus, [bins[2]], None, "the withheld block")
        assert got.n_connected == 45 and engine.pending_stats().levels == ROUNDS
    finally:
        engine.index_clear()


# ---------------------------------------------------------------- 10. mixing
def test_accept_on_the_same_context(eng, corpus):
    """mv_accept_blocks reads KNOWN as HAVE or STORED, and parks nothing."""
    bins = corpus[0]
    three = model(corpus, eng)
    connect(eng, three, corpus, bins[0:4] + bins[8:12], None, "rounds 1 and 3")
    got, want = eng.accept_blocks(bins[0:12]), three.accept(bins[0:12])
    assert got.blk_state.tolist() == want.blk_state == [M.ACC_KNOWN] * 4 + [M.ACC_NEW] * 4 + [M.ACC_KNOWN] * 4
    assert got.n_missing == want.n_missing == 0
    check_state(eng, three, all_refs(corpus), "accept")  # round 2 is HAVE and not in the store: the sweep never sees it
    got, _ = connect(eng, three, corpus, (), None, "sweep")
    assert got.n_connected == 0 and eng.pending_stats().suspended == 4
    eng.index_clear()
    ps = eng.pending_stats()
    assert (ps.stored, ps.suspended, ps.includes, ps.levels) == (0, 0, 0, 0)
    three = model(corpus, eng)
    got, _ = connect(eng, three, corpus, bins[0:8], None, "after the clear")
    assert got.n_connected == 8


def test_stored_is_refused_by_index_insert_and_taken_by_the_device_insert(eng, corpus):
    import torch

    refs = rand_refs(random.Random(3), 5)
    with pytest.raises(M.MvError, match=r"\(-1\)"):
        eng.index_insert(refs, M.REF_STORED)
    assert eng.index_insert(refs[:2], M.REF_WANTED).tolist() == [0, 0]
    assert eng.index_insert(refs[2:3], M.REF_HAVE).tolist() == [0]
    eng.index_reserve(64)
    d_words = torch.from_numpy(IM.ref_words(refs[1:]).view(np.int64).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    eng.dev_index_insert(0, d_words, 6, 4, M.REF_STORED)
    assert eng.index_lookup(refs).tolist() == [1, 3, 3, 3, 3]
    assert eng.index_insert_stored(refs).tolist() == [1, 3, 3, 3, 3]
    st, ps = eng.index_stats(), eng.pending_stats()
    assert (st.have, st.wanted, ps.stored) == (5, 0, 5)
    assert eng.index_insert(refs, M.REF_HAVE).tolist() == [3] * 5 and eng.index_lookup(refs).tolist() == [3] * 5


def test_resources_return_after_destroy(engine, corpus):
    bins = corpus[0]
    base = engine.get_option("MV_LIVE_RESOURCES")
    e = M.Engine(devices=(0,))
    try:
        e.set_committee(*corpus[1])
        ps = e.pending_stats()
        assert (ps.stored, ps.suspended, ps.includes, ps.levels) == (0, 0, 0, 0)  # no index yet: nothing is made
        assert e.connect_blocks().n_connected == 0
        with_committee = engine.get_option("MV_LIVE_RESOURCES")
        e.index_insert_stored(corpus[2])
        assert e.connect_blocks(bins[4:12]).n_connected == 0 and e.pending_stats().suspended == 8
        e.pending_reserve(1000, 10000)  # grows with records in it
        assert e.connect_blocks(bins[0:4]).n_connected == 12
        assert engine.get_option("MV_LIVE_RESOURCES") > with_committee
    finally:
        e.close()
    assert engine.get_option("MV_LIVE_RESOURCES") == base
