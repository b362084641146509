"""GPU: the decision rule, the commit sequence, the replay summary and the recovery at committees of up
to 512 seats -- every word of the 16-word blame, vote and certificate bitmaps, every pass of
bitmap_stake, both strides of the replay summary's seen[] -- on the small DAGs of
tests/wide_committee.py, whose stakes are skewed so that a quorum needs a dozen includes. Every row's
eight words and three stakes are compared with commit_model.DirectRule, the commit rows, info words
and sequence length with commit_seq_model.CommitRule, last_seen_by_authority with replay_model and the
seeded store with recover_model: never with another device form. Tag widths 64 and 2.
tests/test_wide_committee_model.py holds the cases themselves to the oracle and the models to each other."""
import random

import numpy as np
import pytest

import commit_model as C
import index_model as IM
import mysticeti_amd as M
import replay_model as RM
import wal as WAL
import wide_committee as W
from test_gpu_commit import check, deliver, rule_of
from test_gpu_decide import check_rows, deliver_and_check, model_of, store_engine, tag  # noqa: F401
from test_gpu_index import rand_refs
from test_gpu_recover import blank, genesis_bins, rec_engine, recover, verdicts_of  # noqa: F401

pytestmark = pytest.mark.gpu

_built = {}


@pytest.fixture
def case(engine):
    """case(name): the case, built and signed once."""
    def get(name):
        if name not in _built:
            _built[name] = W.CASES[name](engine)
        return _built[name]

    return get


DECIDE_CASES = [n for n in W.CASES if not n.startswith("sequence")]


# ---------------------------------------------------------------- 1. the direct rule, case by case
@pytest.mark.parametrize("name", DECIDE_CASES)
def test_rows(store_engine, case, tag, name):
    c = case(name)
    got, want = deliver_and_check(store_engine, tag, c.dag, c.leaders, name)
    if name == "one_blame":
        assert got.status.tolist() == [M.LEADER_COMMIT] * 16
        assert [int(s) for s in got.stakes[:, 0]] == [c.plan.stakes[a] for a in W.WORD_BLAMERS]
    if name in ("blame_edge", "quorum_edge"):
        col = 0 if name == "blame_edge" else 2
        assert {w.stakes[col] for w in want} == {c.plan.thr, c.plan.thr + 1}
    if name.startswith("top_"):
        assert want[0].stakes[0 if "blame" in name else 2] == c.plan.thr + 1


# ---------------------------------------------------------------- 2. the commit sequence
@pytest.mark.parametrize("which", ["sequence_linked", "sequence_unlinked"])
def test_commit_sequence(store_engine, case, tag, which):
    c, e = case(which), store_engine
    deliver(e, tag, c.dag)
    got = e.commit_leaders(c.leaders)
    want = check(got, rule_of(c.dag.stakes, c.dag.blocks, list(c.dag.blocks)), c.leaders, which)
    w = want[(480, 5)]
    assert (w.status, w.kind, c.leaders[w.anchor]) == (C.COMMIT if which == "sequence_linked" else C.SKIP, 2, (511, 8))
    assert got.n_sequence == len(c.leaders) == 48


# ---------------------------------------------------------------- 3. after a prune, after a rebuild
def test_after_a_prune(store_engine, case, tag):
    c, e = case("one_blame"), store_engine
    deliver_and_check(e, tag, c.dag, c.leaders)
    e.dag_prune(2)  # the leader round stays
    kept = [r for r in c.dag.blocks if r[1] >= 2]
    st = e.dag_stats()
    assert (st.records, st.lowest_round, st.highest_round) == (len(kept), 2, 4) and len(kept) < len(c.dag.blocks)
    want = check_rows(e.decide_leaders(c.leaders), model_of(c.dag.stakes, c.dag.blocks, kept), c.leaders, "pruned at 2")
    assert [w.status for w in want] == [C.COMMIT] * 16
    e.dag_prune(3)  # ... and now it is below the lowest round
    kept = [r for r in c.dag.blocks if r[1] >= 3]
    want = check_rows(e.decide_leaders(c.leaders), model_of(c.dag.stakes, c.dag.blocks, kept), c.leaders, "pruned at 3")
    assert [w.status for w in want] == [C.UNDECIDED] * 16


def test_after_a_rebuild(case, tag):
    c = case("one_blame")
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(1)
        e.dag_reserve(1, 1)
        deliver_and_check(e, tag, c.dag, c.leaders, "grown")
        rng, rebuilds = random.Random(8), e.index_stats().rebuilds
        assert rebuilds >= 1
        while e.index_stats().rebuilds == rebuilds:
            e.index_insert(rand_refs(rng, 100), M.REF_WANTED)
        check_rows(e.decide_leaders(c.leaders), model_of(c.dag.stakes, c.dag.blocks, list(c.dag.blocks)), c.leaders,
                   "after the rebuild")
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the device-buffer calls
def test_device_buffer_calls(store_engine, case, tag):
    import torch

    c, e = case("one_blame"), store_engine
    deliver(e, tag, c.dag)
    dev = torch.device("cuda", 0)
    n = len(c.leaders)
    d_lead = torch.from_numpy(np.asarray(c.leaders, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_out = torch.full((n + 1, 8), -3, dtype=torch.int64, device=dev)
    d_stakes = torch.full((n + 1, 3), -3, dtype=torch.int64, device=dev)
    d_info = torch.full((n + 1, 4), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    e.dev_decide_leaders(0, d_lead, d_out[:n], d_stakes[:n])
    out, stakes = d_out.cpu().numpy(), d_stakes.cpu().numpy()
    assert (out[n:] == -3).all() and (stakes[n:] == -3).all()
    got = M.Decided(out[:n].view(np.uint64), stakes[:n].view(np.uint64))
    check_rows(got, model_of(c.dag.stakes, c.dag.blocks, list(c.dag.blocks)), c.leaders, "mv_dev_decide_leaders")
    d_out.fill_(-3)
    torch.cuda.synchronize(dev)
    n_seq = e.dev_commit_leaders(0, d_lead, d_out[:n], d_info[:n])
    out, info = d_out.cpu().numpy(), d_info.cpu().numpy()
    assert (out[n:] == -3).all() and (info[n:] == -3).all()
    got = M.Committed(out[:n].view(np.uint64), info[:n].view(np.uint64), n_seq, np.asarray(c.leaders, dtype=np.uint64))
    check(got, rule_of(c.dag.stakes, c.dag.blocks, list(c.dag.blocks)), c.leaders, "mv_dev_commit_leaders")
    assert n_seq == 16


# ---------------------------------------------------------------- 5. replay and recover
NAMED, ABSENT = (0, 255, 256, 300, 510, 511), (1, 257, 509)
BITS = 16


def by_round(dag, rounds):
    return [dag.blocks[ref][0] for r in rounds for ref in sorted(dag.rounds[r])]


def image_of(parts):
    """A WAL of the parts in order: a list of blocks, or None for an entry of an unknown tag."""
    w = WAL.WalWriter(BITS)
    k = 0
    for part in parts:
        if part is None:
            w.write(9, b"what")
            continue
        for b in part:
            w.write(2, bytes([k & 255]) * (k % 8))
            w.write(1, b)
            k += 1
    return w.image(), w.pos


def device_last_seen(e, img, end, n_auth):
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
             d_last_seen=torch.full((n_auth + 2,), -3, dtype=torch.int64, device=dev))
    torch.cuda.synchronize(dev)
    counts = e.dev_wal_replay(0, d_img, size, end, BITS, **o)
    seen = o["d_last_seen"].cpu().numpy()
    assert (seen[n_auth:] == -3).all()
    return counts, seen[:n_auth].view(np.uint64), o["d_summary"].cpu().numpy().view(np.uint64)


def test_replay_summary_of_512_seats(rec_engine, case):
    """Every producer's blocks stand with the higher round first. The cut image ends in an entry of an
    unknown tag ahead of seat 511's second block, with rounds 4 and 3 behind it: what the summary must not read."""
    c, e = case("one_blame"), rec_engine
    dag = c.dag
    assert all(sum(ref[0] == a for ref in dag.blocks) == 4 for a in NAMED) and not any(ref[0] in ABSENT for ref in dag.blocks)
    blank(e, 64, dag)
    whole = [genesis_bins(dag.n), by_round(dag, (4, 3, 2, 1))]
    r1 = by_round(dag, (1,))
    cut = [genesis_bins(dag.n), by_round(dag, (2,)), r1[:-1], None, r1[-1:], by_round(dag, (4, 3))]
    assert IM.own_ref(r1[-1])[:2] == (511, 1)
    for what, parts, top in (("whole", whole, 4), ("cut", cut, 2)):
        img, end = image_of(parts)
        want = RM.model(img, end, BITS, dag.n, verdicts_of(dag))
        assert want.last_seen.tolist() == [top if a in W.PRODUCERS else 0 for a in range(512)], what
        assert (want.status[-1] == RM.UNKNOWN_TAG) == (what == "cut") and want.n_blocks == 512 + 34 * top - (what == "cut")
        RM.assert_same(e.wal_replay(img, end_pos=end, map_bits=BITS), want, "mv_wal_replay, " + what)
        counts, seen, summary = device_last_seen(e, img, end, dag.n)
        assert counts == (want.count, want.n_blocks), what
        assert seen.tolist() == want.last_seen.tolist() and summary.tolist() == want.summary.tolist(), what


def test_recover_then_decide(rec_engine, case, tag):
    c, e = case("one_blame"), rec_engine
    dag = c.dag
    blank(e, tag, dag)
    model, seeded, want = recover(e, dag, genesis_bins(dag.n) + by_round(dag, (4, 3, 2, 1)), bits=BITS)
    assert seeded.records == len(dag.bins) and seeded.wanted == 0 and (want.blk_status[512:] == M.BLOCK_OK).all()
    d = C.DirectRule(dag.stakes)
    for ref, incs in model.records:
        d.add(ref, incs)
    rows = check_rows(e.decide_leaders(c.leaders), d, c.leaders, "recovered")
    assert [w.status for w in rows] == [C.COMMIT] * 16
    check(e.commit_leaders(c.leaders), model.rule(dag.stakes), c.leaders, "recovered")
