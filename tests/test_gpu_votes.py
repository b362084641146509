"""mv_aggregate_votes against the per-cell rule (votes_model.CellRule): per-block counts, flags,
certified rows and their order, and the store's statistics, exactly."""
import numpy as np
import pytest

import mysticeti_amd as M
import votes_cases as vc
from mysticeti_amd import blocks as MB
from votes_model import CellRule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def one_key(engine):
    return MB.committee(engine, 1, False)[0][0]


def make_engine(one_key, stakes, reserve=(4096, 1 << 16)):
    e = M.Engine(devices=(0,))
    e.set_committee(np.tile(one_key, (len(stakes), 1)), np.asarray(stakes, dtype=np.uint64))
    if reserve:
        e.votes_reserve(*reserve)
    return e


@pytest.fixture
def make(one_key):
    made = []

    def fn(stakes, reserve=(4096, 1 << 16)):
        made.append(make_engine(one_key, stakes, reserve))
        return made[-1]

    yield fn
    for e in made:
        e.close()


def expect(model, blocks, register_only=False):
    """What CellRule says of one call: counts (n x 4) and the certified rows."""
    counts, rows = [], []
    for i, b in enumerate(blocks):
        r = model.process_block(b, register_only)
        counts.append([len(r.processed), r.unknown, r.duplicate, r.flags])
        rows += [list(vc.ref_words(ref)) + [o, i] for ref, o in r.processed]
    return counts, rows


def check_stats(e, model, what=""):
    st = e.votes_stats()
    assert (st.pending, st.aggregating, st.certified) == (model.len(), model.aggregating(), model.certified), \
        (what, st.as_tuple(), model.len(), model.aggregating(), model.certified)
    return st


def call(e, model, blocks, register_only=False, what=""):
    counts, rows = expect(model, blocks, register_only)
    st, got_counts, got_rows, total = e.aggregate_votes([vc.encode_block(b) for b in blocks], register_only,
                                                        cap_certified=len(rows) + 3)
    assert st.tolist() == [M.VOTES_OK] * len(blocks), what
    assert got_counts.tolist() == counts, (what, got_counts.tolist(), counts)
    assert total == len(rows) and got_rows.tolist() == rows, (what, total, len(rows))
    return check_stats(e, model, what)


@pytest.mark.parametrize("name", sorted(vc.named_cases()))
def test_named_case(make, name):
    """Shares interleaved with votes, the exact threshold, a voter twice, a single-authority quorum,
    order inside a call, VoteRange and Vote edges, a block twice, register-only, wide ranges."""
    stakes, calls = vc.named_cases()[name]
    e, model = make(stakes), CellRule(stakes)
    for k, (blocks, register_only) in enumerate(calls):
        call(e, model, blocks, register_only, what=(name, k))


def test_named_cases_say_what_they_claim():
    """The figures the cases are named after, from the model: they are what the GPU is compared with."""
    cases = vc.named_cases()
    stakes, calls = cases["interleaved"]
    counts, rows = expect(CellRule(stakes), calls[0][0])
    assert counts[0] == [0, 3, 0, 0]                        # its own votes: an unseen block
    assert [c[1] for c in counts[1:]] == [2, 2, 5]          # offsets 1 and 4 are not Shares; the third votes after certification
    assert [r[6:] for r in rows] == [[0, 2], [2, 2], [3, 2]]  # certified by the second voter (quorum 3)
    stakes, calls = cases["threshold_exact"]
    m = CellRule(stakes)
    assert vc.quorum(stakes) == 9
    assert [c[0] for c in expect(m, calls[0][0])[0]] == [0, 0, 1] and [c[0] for c in expect(m, calls[1][0])[0]] == [1]
    stakes, calls = cases["threshold_one_less"]
    assert sum(c[0] for c in expect(CellRule(stakes), calls[0][0])[0]) == 0
    stakes, calls = cases["single_quorum"]
    m = CellRule(stakes)
    assert expect(m, calls[0][0])[0] == [[0, 0, 0, 0]] and [c[0] for c in expect(m, calls[1][0])[0]] == [1, 1]
    stakes, calls = cases["order_in_call"]
    counts, rows = expect(CellRule(stakes), calls[0][0])
    assert counts[0][:2] == [0, 3] and counts[2][:2] == [0, 0] and {r[7] for r in rows} == {7}
    assert [c[:2] for c in counts[8:]] == [[0, 3]] * 3      # votes after certification
    stakes, calls = cases["vote_edges"]
    assert expect(CellRule(stakes), calls[0][0])[0][1][3] == M.VOTES_FLAG_REJECT | M.VOTES_FLAG_OFFSET | M.VOTES_FLAG_RANGE


@pytest.mark.parametrize("n_auth", [65, 512])
def test_voter_words(make, n_auth):
    """Committees that cross the 64-bit word edges of the voter set: voters 0, 63, 64 and the last,
    twice each, then enough of the others to certify."""
    stakes = [1] * n_auth
    e, model = make(stakes), CellRule(stakes)
    b = vc.block(63, 1, vc.shares(3))
    edge = [0, 63, 64, n_auth - 1]
    votes = [vc.block(a, 2, [("range", b[1], 0, 2)], tag=k) for k in range(2) for a in edge]
    call(e, model, [b] + votes)
    rest = [a for a in range(n_auth) if a not in edge][:vc.quorum(stakes)]
    st = call(e, model, [vc.block(a, 3, [("range", b[1], 0, 3)]) for a in rest])
    assert st.certified == 3 and st.pending == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_call_per_block_and_every_split(make, seed):
    """The same blocks in one call, one call per block and split at every position: identical
    results and statistics."""
    stakes = vc.unequal_stakes(5)
    blocks = vc.random_blocks(seed, 5, 12)
    bins = [vc.encode_block(b) for b in blocks]
    model = CellRule(stakes)
    counts, rows = expect(model, blocks)
    e = make(stakes)
    for cuts in [[0, len(blocks)], list(range(len(blocks) + 1))] + [[0, k, len(blocks)] for k in range(1, len(blocks))]:
        e.votes_clear()
        e.votes_reserve(64, 1024)
        got_counts, got_rows = [], []
        for lo, hi in zip(cuts, cuts[1:]):
            st, c, r, total = e.aggregate_votes(bins[lo:hi], cap_certified=256)
            assert total == len(r)
            r[:, 7] += lo
            got_counts += c.tolist()
            got_rows += r.tolist()
        assert got_counts == counts and got_rows == rows, cuts
        check_stats(e, model, cuts)


def test_parse_errors_change_nothing(make):
    """Every truncation of one small block, between two good neighbours."""
    stakes = [1, 1, 1, 1]
    e, model = make(stakes), CellRule(stakes)
    b = vc.block(0, 1, vc.shares(2))
    v1, v2 = (vc.block(a, 2, [("range", b[1], 0, 2), ("vote", b[1], 0)]) for a in (1, 2))
    call(e, model, [b])
    whole = vc.encode_block(v1)
    cuts = [whole[:k] for k in range(len(whole))]
    st, counts, rows, total = e.aggregate_votes([vc.encode_block(v1)] + cuts + [vc.encode_block(v2)], cap_certified=8)
    want = expect(model, [v1, v2])
    assert st.tolist() == [M.VOTES_OK] + [M.VOTES_PARSE_ERROR] * len(cuts) + [M.VOTES_OK]
    assert not counts[1:-1].any()
    assert [counts[0].tolist(), counts[-1].tolist()] == want[0]
    assert [r[:7] for r in rows.tolist()] == [r[:7] for r in want[1]] and rows[:, 7].tolist() == [len(cuts) + 1] * 2
    check_stats(e, model)
    # an author outside the committee
    st, counts, _, _ = e.aggregate_votes([vc.encode_block(vc.block(4, 3, vc.shares(1)))])
    assert st.tolist() == [M.VOTES_UNKNOWN_AUTHOR] and not counts.any()
    check_stats(e, model)


def test_cap_smaller_than_the_total(make):
    stakes = [1, 1, 1, 1]
    e, model = make(stakes), CellRule(stakes)
    b = vc.block(0, 1, vc.shares(9))
    blocks = [b] + [vc.block(a, 2, [("range", b[1], 0, 9)]) for a in (1, 2)]
    counts, rows = expect(model, blocks)
    st, got_counts, got_rows, total = e.aggregate_votes([vc.encode_block(x) for x in blocks], cap_certified=4)
    assert total == 9 and got_rows.tolist() == rows[:4] and got_counts.tolist() == counts
    check_stats(e, model)
    call(e, model, [vc.block(3, 3, [("range", b[1], 0, 9)])])  # all nine are gone: unknown
    # no rows asked for at all
    b2 = vc.block(1, 4, vc.shares(2))
    blocks = [b2] + [vc.block(a, 5, [("range", b2[1], 0, 2)]) for a in (2, 3)]
    expect(model, blocks)
    assert e.aggregate_votes([vc.encode_block(x) for x in blocks], cap_certified=0)[3] == 2
    check_stats(e, model)


def certify_all(e, model, rep, n_auth=4):
    sharing = [vc.block(k % n_auth, 10 * rep + 1, vc.shares(40 + k), tag=k) for k in range(20)]
    votes = [vc.block(a, 10 * rep + 2, [("range", b[1], 0, 64) for b in sharing]) for a in range(n_auth)]
    return call(e, model, sharing + votes, what=rep)


def test_reclamation(make):
    """A workload that certifies everything leaves nothing pending, and repeating it does not raise
    the cells in use above their value after the first repetition."""
    stakes = [1, 1, 1, 1]
    e, model = make(stakes), CellRule(stakes)
    first = certify_all(e, model, 0)
    assert (first.pending, first.aggregating) == (0, 0) and first.certified == sum(40 + k for k in range(20))
    for rep in range(1, 10):
        st = certify_all(e, model, rep)
        assert (st.pending, st.aggregating) == (0, 0) and st.cells_in_use <= first.cells_in_use, rep


def test_growth_from_a_reserve_of_one(make):
    stakes = vc.unequal_stakes(7)
    small, model = make(stakes, reserve=(1, 1)), CellRule(stakes)
    cases_stakes, calls = vc.named_cases()["wide"]
    assert cases_stakes == stakes
    for seed in (5, 6):
        call(small, model, vc.random_blocks(seed, 7, 20), what=seed)
    call(small, model, calls[0][0], what="wide")
    small.votes_reserve(1, 1)  # never shrinks, keeps what is stored
    check_stats(small, model)


def test_device_call(make):
    import torch

    stakes = vc.unequal_stakes(5)
    e, model = make(stakes), CellRule(stakes)
    blocks = vc.random_blocks(11, 5, 25)
    counts, rows = expect(model, blocks)
    dev = torch.device("cuda", 0)
    buf, offs, lens = MB.pack([vc.encode_block(b) for b in blocks] + [b"\0" * 30])  # a short block comes last
    total = int(lens.sum())
    d_buf = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    d_buf[:total] = torch.from_numpy(buf[:total].copy()).to(dev)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)
    n, cap = len(blocks) + 1, len(rows) + 2
    d_st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=dev)
    d_counts = torch.full((n + 2, 4), -3, dtype=torch.int64, device=dev)
    d_rows = torch.full((cap + 2, 8), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    got = e.dev_aggregate_votes(0, d_buf, total, t64(offs), t64(lens), d_st[:n], d_counts[:n], d_rows[:cap])
    st, c, r = d_st.cpu().numpy(), d_counts.cpu().numpy(), d_rows.cpu().numpy()
    assert got == len(rows) and r[:got].tolist() == rows and (r[got:] == -3).all()
    assert st[:n].tolist() == [M.VOTES_OK] * (n - 1) + [M.VOTES_PARSE_ERROR] and (st[n:] == 0xAB).all()
    assert c[:n - 1].tolist() == counts and not c[n - 1].any() and (c[n:] == -3).all()
    check_stats(e, model)


def test_the_block_index_is_not_touched(make):
    """mv_index_stats and an mv_connect_blocks run are the same before and after an aggregate call."""
    stakes = [1, 1, 1, 1]
    e = make(stakes)
    blocks = vc.random_blocks(21, 4, 10)
    bins = [vc.encode_block(b) for b in blocks]
    e.index_reserve(64)
    before = e.connect_blocks(bins)  # (unsigned blocks: rejected, which is a result like any other)
    stats = vars(e.index_stats())
    e.aggregate_votes(bins)
    assert vars(e.index_stats()) == stats
    e.index_clear()
    after = e.connect_blocks(bins)
    assert vars(e.index_stats()) == stats
    assert after.blk_status.tolist() == before.blk_status.tolist() and after.blk_state.tolist() == before.blk_state.tolist()
    assert after.n_connected == before.n_connected and after.n_missing == before.n_missing


def test_documented_errors(one_key):
    e = M.Engine(devices=(0,))
    try:
        bins = [vc.encode_block(vc.block(0, 1, vc.shares(1)))]
        for fn in (lambda: e.votes_reserve(4, 4), lambda: e.aggregate_votes(bins)):
            with pytest.raises(M.MvError) as err:
                fn()
            assert err.value.code == M.E_NO_COMMITTEE
        e.set_committee(np.tile(one_key, (4, 1)), np.ones(4, dtype=np.uint64))
        with pytest.raises(M.MvError) as err:
            e.aggregate_votes(bins)
        assert err.value.code == M.E_INVALID_ARG
        assert e.votes_stats().as_tuple() == (0, 0, 0, 0)
        e.votes_reserve(4, 4)
        assert e.aggregate_votes(bins)[1].tolist() == [[0, 0, 0, 0]]
        assert e.votes_stats().as_tuple() == (1, 1, 1, 0)
        e.votes_clear()
        assert e.votes_stats().as_tuple() == (0, 0, 0, 0)
        with pytest.raises(M.MvError) as err:
            e.aggregate_votes(bins)
        assert err.value.code == M.E_INVALID_ARG
    finally:
        e.close()
