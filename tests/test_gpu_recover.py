"""GPU: mv_wal_recover / mv_dev_dag_seed_rows -- the blocks of a replayed WAL as stored blocks with
records in the DAG store (BlockStore::open with add_unloaded, block_store.rs:50-116, 398-404) -- against
tests/recover_model.py over the rows of tests/replay_model.py, with the CPU oracle's block verdicts.
What the store then holds is read through mv_commit_leaders and compared, array for array, with
tests/commit_seq_model.py's CommitRule fed with the model's records, and with a context that got the
same blocks through mv_connect_blocks. DAGs are built, signed and delivered as tests/test_gpu_decide.py
and tests/test_gpu_commit.py do; images come from oracle/wal.py's WalWriter, with a tag-2 entry of
0..7 bytes ahead of every block (blocks start at every offset mod 8) and every fourth block an own
block (tag 3: 8 bytes further on)."""
import random
import struct

import numpy as np
import pytest

import commit_model as C
import commit_seq_model as S
import connect_model as CM
import index_model as IM
import mysticeti_amd as M
import recover_model as RC
import replay_model as RM
import wal as W
from mysticeti_amd import blocks as MB
from test_gpu_commit import check, random7, rows_of, valid_random_dag  # noqa: F401
from test_gpu_decide import Dag, ready, store_engine, tag  # noqa: F401
from test_gpu_index import rand_refs
from test_gpu_replay import bad_signature

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec_engine():
    """The context that restarts: a DAG store, and nothing in it but what a test recovers."""
    e = M.Engine(devices=(0,))
    e.dag_reserve(64, 256)
    yield e
    e.close()


def genesis_bins(n_auth):
    return [MB.encode(a, 0, [], [], [], 0, 0, bytes(64), d)[0] for a, _, d in MB.genesis_refs(n_auth)]


def wal_of(blocks, bits=12):
    w = W.WalWriter(bits)
    for k, b in enumerate(blocks):
        w.write(2, bytes([k & 255]) * (k % 8))
        w.write(3 if k % 4 == 3 else 1, (struct.pack("<Q", k) if k % 4 == 3 else b"") + b)
    return w.image(), w.pos


def verdicts_of(dag):
    return RM.oracle_verdicts(dag.pks, np.asarray(dag.stakes, dtype=np.uint64), 0)


def blank(e, tag, dag):
    """A cleared context with the committee: genesis comes from the WAL, as in Core::open (core.rs:97-113)."""
    e.set_committee(dag.pks, np.asarray(dag.stakes, dtype=np.uint64), 0)
    e.set_option("MV_INDEX_TAG_BITS", tag)
    e.index_clear()


def stats_of(e):
    st = e.dag_stats()
    return (st.records, st.includes, st.lowest_round, st.highest_round)


def recover(e, dag, blocks, floor=0, bits=12, store=None):
    """mv_wal_recover of the blocks' WAL: its replay outputs, the five words and mv_dag_stats against the models."""
    img, end = wal_of(blocks, bits)
    rep, seeded = e.wal_recover(img, end_pos=end, map_bits=bits, floor_round=floor)
    want = RM.model(img, end, bits, dag.n, verdicts_of(dag))
    RM.assert_same(rep, want, "the replay of mv_wal_recover")
    model = RC.Store() if store is None else store
    words = model.seed(img, want.rows, want.blk_status, floor)
    print(f"recover: rows {want.n_blocks}, seeded {seeded.words()}, model {words}, stats {stats_of(e)}")
    assert seeded.words() == words
    assert stats_of(e) == model.stats()
    return model, seeded, want


def connect_all(e, tag, dag, bins=None):
    """The blocks through mv_connect_blocks in one call -> the references in connected-row order."""
    ready(e, tag, dag.pks, dag.stakes, dag.n)
    bins = list(dag.bins if bins is None else bins)
    c = e.connect_blocks(bins)
    assert c.n_connected == len(bins)
    return [IM.words_ref(r[:6]) for r in c.connected]


def same(a, b):
    return np.array_equal(a.rows, b.rows) and np.array_equal(a.info, b.info) and a.n_sequence == b.n_sequence


# ---------------------------------------------------------------- 1. restart equals no restart
def test_restart_equals_no_restart(store_engine, rec_engine, random7, tag):
    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    order = connect_all(store_engine, tag, dag)
    live, live_stats = store_engine.commit_leaders(leaders), stats_of(store_engine)
    blank(e, tag, dag)
    model, seeded, want = recover(e, dag, genesis_bins(dag.n) + [dag.blocks[r][0] for r in order])
    assert set((want.rows[:, 1] % 8).tolist()) == set(range(8)) and (want.rows[:, 9] != M.WAL_NONE).sum() == len(want.rows) // 4
    assert seeded.words() == [dag.n + len(order), len(order), sum(len(dag.blocks[r][1]) for r in order), 0, 0]
    assert [r for r, _ in model.records] == order
    got = e.commit_leaders(leaders)
    check(got, model.rule(dag.stakes), leaders, "recovered")
    assert same(got, live) and stats_of(e) == live_stats
    assert e.pending_stats().stored == store_engine.pending_stats().stored == dag.n + len(order)
    assert e.index_wanted()[1] == 0


# ---------------------------------------------------------------- 2. it fails without the feature
def test_the_old_seeding_decides_nothing(rec_engine, random7):
    import torch

    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    img, end = wal_of(genesis_bins(dag.n) + dag.bins)
    blank(e, 64, dag)
    rep = e.wal_replay(img, end_pos=end, map_bits=12)
    e.index_reserve(2 * rep.n_blocks)
    d_rows = torch.from_numpy(rep.rows.view(np.int64).copy()).to(torch.device("cuda", 0))
    e.dev_index_insert(0, d_rows, 10, rep.n_blocks, M.REF_STORED, word_offset=3)
    old = e.commit_leaders(leaders)
    assert e.pending_stats().stored == rep.n_blocks and stats_of(e) == (0, 0, 0, 0)
    assert not np.isin(old.status, (M.LEADER_COMMIT, M.LEADER_SKIP)).any() and old.n_sequence == 0
    blank(e, 64, dag)
    model, _, _ = recover(e, dag, genesis_bins(dag.n) + dag.bins)
    got = e.commit_leaders(leaders)
    want = check(got, model.rule(dag.stakes), leaders, "recovered")
    kinds = [(w.status, w.kind) for w in want.values()]
    assert (C.COMMIT, 1) in kinds and (C.COMMIT, 2) in kinds and (C.SKIP, 2) in kinds and got.n_sequence > 0


# ---------------------------------------------------------------- 3. recovery, then live traffic
def recovered_then_live(e, tag, dag, order, rebuild):
    early = [r for r in order if r[1] <= 8]
    late = [dag.blocks[r][0] for r in order if r[1] > 8]
    blank(e, tag, dag)
    model, _, _ = recover(e, dag, genesis_bins(dag.n) + [dag.blocks[r][0] for r in early])
    if rebuild:
        rng, rebuilds = random.Random(8), e.index_stats().rebuilds
        while e.index_stats().rebuilds == rebuilds:
            e.index_insert(rand_refs(rng, 100), M.REF_WANTED)
    random.Random(len(late)).shuffle(late)
    c = e.connect_blocks(late)
    assert c.n_connected == len(late) and c.n_missing == 0
    for row in c.connected:
        ref = IM.words_ref(row[:6])
        model.add_record(ref, dag.blocks[ref][1])
    assert stats_of(e) == model.stats()
    return model


def test_recovery_then_live_traffic(store_engine, rec_engine, random7, tag):
    dag = random7
    leaders = rows_of(S.PIPELINED_TWO, dag)
    order = connect_all(store_engine, tag, dag)
    live, live_stats = store_engine.commit_leaders(leaders), stats_of(store_engine)
    model = recovered_then_live(rec_engine, tag, dag, order, rebuild=False)
    got = rec_engine.commit_leaders(leaders)
    check(got, model.rule(dag.stakes), leaders, "recovered, then connected")
    assert same(got, live) and stats_of(rec_engine) == live_stats


def test_recovery_a_rebuild_then_live_traffic(store_engine, random7):
    dag = random7
    leaders = rows_of(S.PIPELINED_TWO, dag)
    order = connect_all(store_engine, 2, dag)
    live = store_engine.commit_leaders(leaders)
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(8)
        e.dag_reserve(2, 2)
        model = recovered_then_live(e, 2, dag, order, rebuild=True)
        got = e.commit_leaders(leaders)
        check(got, model.rule(dag.stakes), leaders, "recovered, rebuilt, then connected")
        assert same(got, live)
    finally:
        e.close()


# ---------------------------------------------------------------- 4. eligibility edges
@pytest.fixture(scope="module")
def rejected4(engine):
    """Four authorities; (3, 2) is in the WAL with a bad signature only, and round 3 includes that block."""
    d = Dag(engine, 4, [1] * 4, distinct=False)
    d.full()
    r2 = d.full()
    bad = bad_signature(d.blocks[r2[3]][0])
    bad_ref = IM.own_ref(bad)
    d.layer([(a, r2[:3] + [bad_ref]) for a in range(4)])
    for _ in range(4):
        d.full()
    return d, r2[3], bad, bad_ref


def test_a_rejected_block_is_stored_without_a_record(rec_engine, rejected4, tag):
    (dag, gone, bad, bad_ref), e = rejected4, rec_engine
    leaders = rows_of(S.PIPELINED, dag)
    blocks = genesis_bins(4) + [bad if b is dag.blocks[gone][0] else b for b in dag.bins]
    blank(e, tag, dag)
    model, seeded, want = recover(e, dag, blocks)
    assert want.blk_status.tolist().count(M.BLOCK_SIG_INVALID) == 1 and seeded.records == len(dag.bins) - 1
    assert e.index_lookup([bad_ref, gone]).tolist() == [M.REF_STORED, M.REF_ABSENT] and seeded.wanted == 0
    assert all(r != bad_ref for r, _ in model.records) and sum(bad_ref in i for _, i in model.records) == 4
    check(e.commit_leaders(leaders), model.rule(dag.stakes), leaders, "a rejected block")


def test_a_block_written_twice_and_a_reference_with_a_record(rec_engine, random7, tag):
    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    blocks = genesis_bins(dag.n) + dag.bins[:30] + [dag.bins[11], dag.bins[3]] + dag.bins[30:] + [dag.bins[50]]
    blank(e, tag, dag)
    model, seeded, _ = recover(e, dag, blocks)
    assert seeded.rows == dag.n + len(dag.bins) + 3 and seeded.records == len(dag.bins)
    full = e.commit_leaders(leaders)
    check(full, model.rule(dag.stakes), leaders, "written twice")
    # round 1 through a connect call first: its references have records when the WAL is recovered
    ready(e, tag, dag.pks, dag.stakes, dag.n)
    first = [dag.blocks[r][0] for r in dag.rounds[1]]
    c = e.connect_blocks(first)
    assert c.n_connected == len(first)
    model = RC.Store(dag.genesis)
    for row in c.connected:
        ref = IM.words_ref(row[:6])
        model.add_record(ref, dag.blocks[ref][1])
    _, seeded, _ = recover(e, dag, genesis_bins(dag.n) + dag.bins, store=model)
    assert seeded.records == len(dag.bins) - len(first) and len(model.records) == len(dag.bins)
    assert same(e.commit_leaders(leaders), full)


def test_floor_round_around_a_voting_round(rec_engine, random7, tag):
    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    for floor in (5, 6, 7):  # the voting round of the leaders of round 5 is 6
        blank(e, tag, dag)
        model, seeded, _ = recover(e, dag, genesis_bins(dag.n) + dag.bins, floor=floor)
        assert [r for r, _ in model.records] == [r for r in dag.blocks if r[1] >= floor] and seeded.wanted == 0
        got = e.commit_leaders(leaders)
        check(got, model.rule(dag.stakes), leaders, f"floor {floor}")
        # what mv_dag_prune(floor) leaves of the whole store
        blank(e, tag, dag)
        recover(e, dag, genesis_bins(dag.n) + dag.bins)
        e.dag_prune(floor)
        assert stats_of(e) == model.stats() and same(e.commit_leaders(leaders), got)


# ---------------------------------------------------------------- 5. wide and many
@pytest.fixture(scope="module")
def wide2(engine):
    """70 authorities: (4, 3) has 65 includes, (5, 4) has 130 -- round 3 and weak links to round 2."""
    n = 70
    d = Dag(engine, n, [1] * n, distinct=True)
    d.full()
    r2 = d.full()
    r3 = d.layer([(a, r2[:65] if a == 4 else r2) for a in range(n)])
    d.layer([(a, r3 + r2[:60] if a == 5 else r3) for a in range(n)])
    d.full()
    d.full()
    return d


def test_wide_blocks(rec_engine, wide2):
    dag, e = wide2, rec_engine
    assert len(dag.blocks[dag.first(3)[4]][1]) == 65 and len(dag.blocks[dag.first(4)[5]][1]) == 130
    leaders = rows_of(S.PIPELINED, dag)
    blank(e, 64, dag)
    model, seeded, want = recover(e, dag, genesis_bins(dag.n) + dag.bins, bits=16)
    assert want.blk_status.tolist() == [M.BLOCK_GENESIS] * 70 + [M.BLOCK_OK] * 420 and seeded.records == 420
    got = e.commit_leaders(leaders)
    res = check(got, model.rule(dag.stakes), leaders, "wide")
    assert res[(2, 2)].status == C.COMMIT and res[(3, 3)].status == C.COMMIT


@pytest.fixture(scope="module")
def long7(engine):
    d = Dag(engine, 7, [1] * 7, distinct=True)
    refs = {(a, 0, 0): d.genesis[a] for a in range(7)}
    for rnd, layer in enumerate(valid_random_dag(5, 7, 40), 1):
        made, seen = d.layer([(a, [refs[i] for i in incs]) for a, incs in layer]), {}
        for (a, _), ref in zip(layer, made):
            refs[(a, rnd, seen.get(a, 0))] = ref
            seen[a] = seen.get(a, 0) + 1
    return d


def test_many_rows(rec_engine, long7):
    dag, e = long7, rec_engine
    assert len(dag.bins) > 256
    blank(e, 64, dag)
    model, seeded, want = recover(e, dag, genesis_bins(dag.n) + dag.bins)
    assert seeded.records == len(dag.bins) and (want.blk_status[7:] == M.BLOCK_OK).all()
    leaders = [x for x in rows_of(S.PIPELINED_TWO, dag) if 18 <= x[1] <= 22]
    assert len(leaders) == 10
    check(e.commit_leaders(leaders), model.rule(dag.stakes), leaders, "many")


@pytest.fixture(scope="module")
def longer7(engine):
    """80 rounds of 7: 560 records, three workgroups of 256 with the last one partial."""
    d = Dag(engine, 7, [1] * 7, distinct=True)
    refs = {(a, 0, 0): d.genesis[a] for a in range(7)}
    for rnd, layer in enumerate(valid_random_dag(6, 7, 80), 1):
        made, seen = d.layer([(a, [refs[i] for i in incs]) for a, incs in layer]), {}
        for (a, _), ref in zip(layer, made):
            refs[(a, rnd, seen.get(a, 0))] = ref
            seen[a] = seen.get(a, 0) + 1
    return d


def test_records_across_workgroups(rec_engine, longer7):
    """For the leaders around the rounds of records 256 and 512 the voting and decision records, and
    the rounds a walk reads, lie on both sides of a workgroup's edge, in the seeded rows, in the pick
    lists and in the span. Then a prune whose floor cuts through the
    store: what it keeps starts in the second workgroup and fills more than one."""
    dag, e = longer7, rec_engine
    assert len(dag.bins) >= 513
    blank(e, 64, dag)
    blocks = genesis_bins(dag.n) + dag.bins
    model, seeded, want = recover(e, dag, blocks)
    assert seeded.records == len(dag.bins)
    all_leaders = rows_of(S.PIPELINED_TWO, dag)

    def around(store, k):  # the leaders whose voting or decision round holds record k of the store
        r = store.records[k][0][1]
        return [x for x in all_leaders if r - 3 <= x[1] <= r + 1]

    for k in (256, 512):
        leaders = around(model, k)
        assert len(leaders) == 10
        check(e.commit_leaders(leaders), model.rule(dag.stakes), leaders, f"around record {k}")
    floor = 40
    pruned = RC.Store()
    pruned.seed(wal_of(blocks, 12)[0], want.rows, want.blk_status, floor)
    e.dag_prune(floor)
    assert stats_of(e) == pruned.stats() and 256 < pruned.stats()[0] < len(dag.bins) - 256
    leaders = around(pruned, 256)
    assert len(leaders) == 10
    check(e.commit_leaders(leaders), pruned.rule(dag.stakes), leaders, "pruned")


# ---------------------------------------------------------------- 6. a truncated history
def test_truncated_history(rec_engine, random7, tag):
    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    blank(e, tag, dag)
    model, seeded, _ = recover(e, dag, [b for r, (b, _) in dag.blocks.items() if r[1] > 3])
    wanted, n = e.index_wanted()
    assert seeded.wanted == n == len(model.wanted()) > 0
    assert {IM.words_ref(w) for w in wanted} == model.wanted() and all(1 <= r[1] <= 3 for r in model.wanted())
    got = e.commit_leaders(leaders)
    want = check(got, model.rule(dag.stakes), leaders, "truncated")
    near = [i for i, x in enumerate(leaders) if x[1] <= 2]  # (their voting round has no record: no quorum of blame either)
    assert all(int(got.status[i]) == M.LEADER_UNDECIDED for i in near)
    assert any(int(got.flags[i]) & M.COMMIT_INCOMPLETE for i in near)
    assert all(w.status != C.SKIP or not w.flags & M.COMMIT_INCOMPLETE for w in want.values())


# ---------------------------------------------------------------- 7. the device variant and refusals
def device_replay(e, img, end, n_auth, bits=12):
    import torch

    dev = torch.device("cuda", 0)
    size, cap, cap_b = len(img), len(img) // 16 + 1, len(img) // 72 + 4
    d_img = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
    d_img[:size] = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).to(dev)
    o = dict(d_pos=torch.full((cap,), -3, dtype=torch.int64, device=dev), d_tag=torch.full((cap,), -3, dtype=torch.int32, device=dev),
             d_len=torch.full((cap,), -3, dtype=torch.int32, device=dev), d_status=torch.full((cap,), 255, dtype=torch.uint8, device=dev),
             d_rows=torch.full((cap_b, 10), -3, dtype=torch.int64, device=dev),
             d_blk_status=torch.full((cap_b,), 255, dtype=torch.uint8, device=dev),
             d_summary=torch.full((3,), -3, dtype=torch.int64, device=dev),
             d_last_seen=torch.full((n_auth,), -3, dtype=torch.int64, device=dev))
    torch.cuda.synchronize(dev)
    _, b = e.dev_wal_replay(0, d_img, size, end, bits, **o)
    assert (o["d_rows"][b:] == -3).all() and (o["d_blk_status"][b:] == 255).all()
    return d_img, o["d_rows"], o["d_blk_status"], b


def index_and_dag(e):
    return tuple(vars(e.index_stats()).values()), stats_of(e), e.pending_stats().stored


def test_device_variant(rec_engine, random7, tag):
    dag, e = random7, rec_engine
    leaders = rows_of(S.PIPELINED_TWO, dag)
    img, end = wal_of(genesis_bins(dag.n) + dag.bins)
    blank(e, tag, dag)
    model, host_seeded, want = recover(e, dag, genesis_bins(dag.n) + dag.bins)
    host, host_stats = e.commit_leaders(leaders), index_and_dag(e)
    blank(e, tag, dag)
    e.index_reserve(4096)
    e.dag_reserve(512, 4096)
    d_img, d_rows, d_st, b = device_replay(e, img, end, dag.n)
    assert b == want.n_blocks
    zero = index_and_dag(e)
    assert e.dev_dag_seed_rows(0, d_img, len(img), d_rows, d_st, n_rows=0).words() == [0] * 5 and index_and_dag(e) == zero
    seeded = e.dev_dag_seed_rows(0, d_img, len(img), d_rows, d_st, n_rows=b)
    assert seeded.words() == host_seeded.words()
    assert (d_rows[b:] == -3).all() and (d_st[b:] == 255).all()
    got = e.commit_leaders(leaders)
    check(got, model.rule(dag.stakes), leaders, "device variant")
    assert same(got, host) and index_and_dag(e)[1:] == host_stats[1:]
    # a row whose length was shortened by hand: a misfit, and nothing else
    k = dag.n + 20
    rows = want.rows.copy()
    rows[k, 2] = 64 + 56 * len(dag.blocks[IM.words_ref(rows[k, 3:9])][1]) - 1
    d_rows[k, 2] = int(rows[k, 2])
    blank(e, tag, dag)
    short = RC.Store()
    words = short.seed(img, rows, want.blk_status)
    assert e.dev_dag_seed_rows(0, d_img, len(img), d_rows, d_st, n_rows=b).words() == words
    assert words[1] == host_seeded.records - 1 and words[3:] == [0, 1] and stats_of(e) == short.stats()
    assert e.pending_stats().stored == b
    check(e.commit_leaders(leaders), short.rule(dag.stakes), leaders, "one misfit")
    # a misaligned image
    with pytest.raises(M.MvError) as err:
        e.dev_dag_seed_rows(0, d_img, len(img) - 4, d_rows, d_st, n_rows=b, img_ptr=d_img.data_ptr() + 4)
    assert err.value.code == M.E_INVALID_ARG


@pytest.mark.parametrize("which", ["index", "store"])
def test_no_room_leaves_index_and_store_unchanged(random7, which):
    dag = random7
    leaders = rows_of(S.PIPELINED_TWO, dag)
    img, end = wal_of(genesis_bins(dag.n) + dag.bins)
    e = M.Engine(devices=(0,))
    try:
        blank(e, 64, dag)
        e.index_reserve(16 if which == "index" else 4096)
        e.dag_reserve(*((512, 4096) if which == "index" else (4, 4)))
        assert e.index_insert_stored(dag.genesis[:2]).tolist() == [0, 0]
        d_img, d_rows, d_st, b = device_replay(e, img, end, dag.n)
        before = index_and_dag(e)
        with pytest.raises(M.MvError) as err:
            e.dev_dag_seed_rows(0, d_img, len(img), d_rows, d_st, n_rows=b)
        assert err.value.code == M.E_INDEX_FULL and index_and_dag(e) == before
        assert e.index_lookup(dag.genesis[:3]).tolist() == [M.REF_STORED, M.REF_STORED, M.REF_ABSENT]
        # the host call grows both
        model, _, _ = recover(e, dag, genesis_bins(dag.n) + dag.bins)
        check(e.commit_leaders(leaders), model.rule(dag.stakes), leaders, "grown")
    finally:
        e.close()


def test_refusals_and_resources(engine, random7):
    dag = random7
    img, end = wal_of(genesis_bins(dag.n) + dag.bins[:20])
    before = engine.get_option("MV_LIVE_RESOURCES")
    e = M.Engine(devices=(0,))
    try:
        with pytest.raises(M.MvError) as err:
            e.wal_recover(img, end_pos=end, map_bits=12)
        assert err.value.code == M.E_NO_COMMITTEE
        e.set_committee(dag.pks, np.asarray(dag.stakes, dtype=np.uint64), 0)
        with pytest.raises(M.MvError) as err:
            e.wal_recover(img, end_pos=end, map_bits=12)
        assert err.value.code == M.E_INVALID_ARG  # no store
        d_img, d_rows, d_st, b = device_replay(e, img, end, dag.n)
        with pytest.raises(M.MvError) as err:
            e.dev_dag_seed_rows(0, d_img, len(img), d_rows, d_st, n_rows=b)
        assert err.value.code == M.E_INVALID_ARG and e.index_stats().have == 0
        e.dag_reserve(8, 8)
        rep, seeded = e.wal_recover(b"", map_bits=12)  # no rows: nothing to seed
        assert (rep.count, rep.n_blocks, seeded.words()) == (0, 0, [0] * 5)
        _, seeded = e.wal_recover(img, end_pos=end, map_bits=12)
        assert seeded.words()[:2] == [dag.n + 20, 20] and engine.get_option("MV_LIVE_RESOURCES") > before
    finally:
        e.close()
    f = M.Engine(devices=(0,))
    try:
        f.dag_reserve(8, 8)
        with pytest.raises(M.MvError) as err:
            f.wal_recover(img, end_pos=end, map_bits=12)
        assert err.value.code == M.E_NO_COMMITTEE
    finally:
        f.close()
    assert engine.get_option("MV_LIVE_RESOURCES") == before


# ---------------------------------------------------------------- 8. untouched neighbours
def test_untouched_neighbours(random7):
    """A context that never calls the new entries: mv_wal_replay's outputs are the model's, its block
    pipeline runs the stages mv_wal_recover's replay runs, and a connect call leaves the counts of
    tests/connect_model.py (no record without mv_dag_reserve)."""
    dag = random7
    blocks = genesis_bins(dag.n) + dag.bins
    img, end = wal_of(blocks)
    want = RM.model(img, end, 12, dag.n, verdicts_of(dag))
    e, r = M.Engine(devices=(0,)), M.Engine(devices=(0,))
    try:
        calls = []
        for x in (e, r):
            blank(x, 64, dag)
            x.set_stage_timing(True)
            x.stage_times(reset=True)
        r.dag_reserve(8, 8)
        RM.assert_same(e.wal_replay(img, end_pos=end, map_bits=12), want, "mv_wal_replay")
        calls.append(e.stage_times(reset=True)[1])
        RM.assert_same(r.wal_recover(img, end_pos=end, map_bits=12)[0], want, "mv_wal_recover")
        calls.append(r.stage_times(reset=True)[1])
        print(f"stage calls: replay {calls[0]}, recover {calls[1]}")
        assert calls[0] == calls[1] and calls[0]["wal_walk"] >= 1
        assert e.index_stats().have == 0 and stats_of(e) == (0, 0, 0, 0)
        three = CM.ThreeState(verdicts_of(dag), dag.genesis)
        m = three.connect(dag.bins)
        assert e.index_insert_stored(dag.genesis).tolist() == [0] * dag.n
        c = e.connect_blocks(dag.bins)
        ps = e.pending_stats()
        assert (ps.stored, ps.suspended, ps.includes, ps.levels) == three.stats() and c.n_connected == m.n_connected
        assert np.array_equal(c.connected, CM.rows_words(m.rows)) and stats_of(e) == (0, 0, 0, 0)
    finally:
        e.close()
        r.close()
