"""GPU: the proposer's state (mv_propose_reserve / add / take / own / stats, mv_dev_propose_add) against
tests/propose_model.py's Core, which tests/test_propose_model.py holds to the reference's text. After
every call its out words, includes, payloads and the stats are compared with the model, at tag widths
64 and 2. Clock-only cases use references seeded into the index; the take, own and end-to-end cases
use blocks signed on the GPU and delivered through connect_blocks, whose records are the model's
block store."""
import random

import numpy as np
import pytest

import connect_model as CM
import index_model as IM
import mysticeti_amd as M
import propose_model as PM
from mysticeti_amd import blocks as MB
from test_gpu_decide import Dag, ready, store_engine, tag  # noqa: F401

pytestmark = pytest.mark.gpu


def words(refs):
    return IM.ref_words(list(refs))


def refs_of(rows):
    return [IM.words_ref(r) for r in rows]


def ref(a, r, salt=0):
    return (a, r, bytes([salt & 255, salt >> 8 & 255]) + bytes(30))


class Pair:
    """The engine's state and the model's, driven by the same calls."""

    def __init__(self, e, stakes, authority=0, entries=8):
        self.e, self.m = e, PM.Core(stakes, authority)
        e.propose_reserve(authority, entries)
        self.outstanding = False
        self.check()

    def check(self):
        assert self.e.propose_stats().words() == self.m.stats(self.outstanding)

    def add(self, refs, tags=None, in_order=False, payload=None, dev=False, stride=6):
        refs = list(refs)
        rows = np.zeros((len(refs), stride), dtype=np.uint64)
        if refs:
            rows[:, :6] = words(refs)
            rows[:, 6:] = 0xDEAD
        if dev:
            import torch

            d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
            d_tags = None if tags is None else torch.from_numpy(np.asarray(tags, dtype=np.uint64).view(np.int64)).cuda()
            got = self.e.dev_propose_add(0, d_rows, d_tags, in_order, payload)
        else:
            got = self.e.propose_add(rows, tags, in_order, payload)
        want = self.m.add_blocks(refs, tags, in_order, payload)
        assert got.words() == want, (refs, in_order)
        self.check()
        return got

    def take(self, cap=1 << 10, cap_p=1 << 10):
        got = self.e.propose_take(cap, cap_p)
        assert got.guard_intact
        want = self.m.try_new_block()
        if want is None:
            assert got.proposed == 0 and got.n_includes == 0 and got.n_payloads == 0
            assert (got.round, got.queue) == (self.m.round, len(self.m.pending))
        else:
            rnd, inc, pay, taken, flags, nxt = want
            assert (got.proposed, got.round, got.taken, got.flags, got.next_entry, got.queue) == \
                (1, rnd, taken, flags, nxt, len(self.m.pending))
            assert got.n_includes == len(inc) and refs_of(got.includes) == inc
            assert got.n_payloads == len(pay) and got.payloads.tolist() == pay
            self.outstanding = True
        self.check()
        return got

    def own(self, r, includes=None):
        got = self.e.propose_own(r, includes)
        assert got.words() == self.m.own_block(r, includes)
        self.outstanding = False
        self.check()
        return got


def seeded(e, tag, stakes, refs):
    """A committee of len(stakes) seats and `refs` in the index (no records)."""
    n = len(stakes)
    pks, _ = MB.committee(e, n, False)
    ready(e, tag, pks, stakes, n)
    if refs:
        e.index_insert_stored(list(refs))


# ---------------------------------------------------------------- the clock
def test_reference_sequence(store_engine, tag):
    """threshold_clock.rs:136-153, a row a call and all in one IN_ORDER call."""
    e = store_engine
    seq = [ref(0, 0), ref(0, 1), ref(1, 0), ref(1, 1), ref(2, 1), ref(3, 1)]
    seeded(e, tag, [1] * 4, seq)
    p = Pair(e, [1] * 4)
    assert [p.add([r]).round for r in seq] == [0, 1, 1, 1, 2, 2]
    seeded(e, tag, [1] * 4, seq)
    p = Pair(e, [1] * 4)
    assert p.add(seq, in_order=True).round == 2
    assert p.add(seq, tags=list(range(6)), dev=True, stride=8).round == 2


def test_greater_ignores_the_quorum(store_engine, tag):
    e = store_engine
    for nxt in (ref(0, 3), ref(1, 3)):
        seeded(e, tag, [7, 1, 1, 1], [ref(0, 3), ref(1, 3)])
        p = Pair(e, [7, 1, 1, 1])
        assert p.add([ref(0, 3)]).round == 3
        assert p.add([nxt]).round == 4


def test_sorted_and_in_order(store_engine, tag):
    e = store_engine
    rows = [ref(0, 2), ref(1, 1), ref(0, 1)]
    for in_order, want in ((False, 3), (True, 2)):
        seeded(e, tag, [7, 1, 1, 1], rows + [ref(0, 0)])
        p = Pair(e, [7, 1, 1, 1])
        assert p.add([ref(0, 0)]).round == 1 and p.m.stake == 0  # seat 0 is a quorum: round 1, an empty set
        assert p.add(rows, tags=[5, 6, 7], in_order=in_order).round == want
        p.own(ref(0, 0, 9), [])  # (the own genesis block, so that a take may run)
        # the queue orders differ accordingly: sorted, the clock is past every entry and the take returns
        # them in queue order; in order, A2 stands in front, at the clock round, and nothing is taken
        got = p.take()
        assert got.proposed == 1
        assert refs_of(got.includes) == [ref(0, 0)] + ([] if in_order else [rows[1], rows[2], rows[0]])
        assert got.next_entry == (5 if in_order else M.PROPOSE_NO_ENTRY)


def test_equivocation_and_fresh_set(store_engine, tag):
    e = store_engine
    a1, a1x, b1, c1, d1 = ref(0, 1), ref(0, 1, 1), ref(1, 1), ref(2, 1), ref(3, 1)
    r2 = [ref(a, 2) for a in range(4)]
    seeded(e, tag, [1] * 4, [a1, a1x, b1, c1, d1] + r2)
    p = Pair(e, [1] * 4)
    assert p.add([a1, a1x, b1]).round == 1 and p.m.stake == 2  # no quorum: an author counts once
    assert p.add([c1]).round == 2
    # one call: the rows behind the quorum row are skipped, the next round starts a fresh set
    seeded(e, tag, [1] * 4, [a1, a1x, b1, c1, d1] + r2)
    p = Pair(e, [1] * 4)
    got = p.add([r2[0], d1, a1, r2[1], a1x, b1, c1])
    assert (got.round, got.voters) == (2, 2)


@pytest.mark.parametrize("n", [5, 33, 512])
def test_quorum_at_word_edges(store_engine, tag, n):
    """The quorum reached by the last seat of a bitmap word and by the first of the next; stakes of 2^40."""
    e = store_engine
    stakes = [1 << 40] * n
    need = 2 * n // 3 + 1
    for last in sorted({31, 32, 63, 64, n - 1} & set(range(n))):
        seats = [a for a in range(n) if a != last][:need - 1] + [last]
        rows = [ref(a, 4) for a in seats]
        seeded(e, tag, stakes, rows)
        p = Pair(e, stakes)
        assert p.add(rows[:-1]).round == 4
        assert p.add(rows[-1:]).round == 5
        seeded(e, tag, stakes, rows)
        p = Pair(e, stakes)
        assert p.add(rows + rows[:3]).round == 5


def test_many_rounds_and_many_rows(store_engine, tag):
    e = store_engine
    rows = [ref(a, r) for r in range(75) for a in range(4)]
    random.Random(7).shuffle(rows)
    seeded(e, tag, [1] * 4, rows)
    p = Pair(e, [1] * 4)
    p.add(rows, tags=list(range(300)))
    # far-off rounds: the sort passes are the bits in which the call's rounds differ, wherever they lie
    far = [ref(1, (1 << 40) + 1), ref(0, 74), ref(2, 1 << 40), ref(3, 1 << 63)]
    e.index_insert_stored(far)
    p.add(far, tags=[1, 2, 3, 4])
    for n in (257, 1025):  # one round, with duplicates: the workgroup and grid edges
        rows = [ref(a % 33, 9, a // 40) for a in range(n)]
        seeded(e, tag, [1] * 33, set(rows))
        p = Pair(e, [1] * 33)
        p.add(rows, dev=(n == 257))


# ---------------------------------------------------------------- the take
def connect(e, p, dag, bins):
    """Delivers blocks; their records join the model's store. Returns the call and its connected references."""
    c = e.connect_blocks(bins)
    rows = refs_of(c.connected[:, :6])
    for r in rows:
        p.m.blocks[r] = list(dag.blocks[r][1])
    return c, rows


def test_cut_and_compression(store_engine, tag):
    e = store_engine
    d = Dag(e, 4, [1] * 4, distinct=False)
    g = d.genesis
    a1, b1, c1, d1 = d.full()
    a2, b2, c2, d2 = d.layer([(0, [a1, b1, c1, d1]), (1, [b1, c1, d1]), (2, [c1, a1, b1, d1]), (3, [d1, c1, b1])])
    ready(e, tag, d.pks, d.stakes, 4)
    p = Pair(e, [1] * 4)
    p.add(g[1:], in_order=True)
    p.own(g[0], [])
    bins = {r: d.blocks[r][0] for r in d.blocks}
    _, rows = connect(e, p, d, [bins[b1], bins[c1]])
    p.add(rows, tags=[21, 22], payload=1001)
    with pytest.raises(M.MvError):
        e.propose_reserve(1, 0)  # reserved for seat 0, and not empty
    # the clock is at 1: the genesis entries are taken (no record, round 0: no flag); b1 is at the cut, and
    # the payload entry behind c1 stays with them
    t = p.take()
    assert (t.proposed, t.taken, t.flags, t.next_entry) == (1, 3, 0, 21) and refs_of(t.includes) == g[1:]
    with pytest.raises(M.MvError):
        e.propose_take()  # a take is outstanding
    p.check()
    p.own(a1)  # [own genesis] + genesis: what Dag.full gave a1
    assert p.m.round == 2
    # records: the own genesis block (no includes), b1, c1, a1
    assert e.dag_stats().records == 4 and e.index_lookup([a1]).tolist() == [M.REF_STORED]
    _, rows = connect(e, p, d, [bins[d1], bins[b2], bins[d2]])
    assert rows == [d1, b2, d2]
    p.add(rows, tags=[23, 24, 25], payload=1002)
    p.add([c1], tags=[26])  # a duplicate queue entry, behind the cut
    # taken: b1 c1 [payload] d1; b2 is the cut (test_payloads_around_the_cut has a payload next to it)
    t = p.take()
    assert (t.taken, t.next_entry) == (4, 24) and refs_of(t.includes) == [b1, c1, d1] and t.payloads.tolist() == [1001]
    p.own(a2)
    assert p.m.round == 3
    _, rows = connect(e, p, d, [bins[c2]])
    p.add(rows + [a2, a2], tags=[27, 28, 29])
    # b2, d2, c2 and the own last block a2 name b1 c1 d1: the duplicate c1 entry is dropped; a2 was queued twice
    # a cap one short of the result: the totals, the rows up to the cap, nothing behind it, the state as it was
    short = e.propose_take(4, 1 << 10)
    assert (short.proposed, short.flags, short.n_includes, short.n_payloads) == (0, M.PROPOSE_SHORT, 5, 1)
    assert refs_of(short.includes) == [b2, d2, c2, a2] and short.guard_intact
    assert (short.taken, short.next_entry, short.queue) == (7, M.PROPOSE_NO_ENTRY, 7)
    p.check()
    short = e.propose_take(1 << 10, 0)
    assert (short.proposed, short.flags, short.n_includes, short.n_payloads) == (0, M.PROPOSE_SHORT, 5, 1)
    assert short.guard_intact and len(short.payloads) == 0
    p.check()
    t = p.take()
    assert refs_of(t.includes) == [b2, d2, c2, a2, a2] and p.m.dropped == 1 and t.payloads.tolist() == [1002]


def test_incomplete_after_prune_and_list_lengths(store_engine, tag):
    """Include lists of 63, 64, 65 and 260 entries (duplicates) under the stamping waves; a pruned round."""
    e = store_engine
    d = Dag(e, 4, [1] * 4, distinct=False)
    g = d.genesis
    r1 = d.full()
    many = [r1[1]] * 63, [r1[2]] * 64, [r1[3]] * 65, [r1[1]] * 260
    r2 = d.layer([(0, r1[:3]), (1, r1[1:] + many[0]), (2, r1[1:] + many[1]), (3, r1[1:] + many[2])])
    d.layer([(1, r2[:3] + many[3]), (2, [r2[1], r2[2], r2[3]]), (3, r2[1:] + [r1[0]])])
    ready(e, tag, d.pks, d.stakes, 4)
    p = Pair(e, [1] * 4)
    p.add(g[1:], in_order=True)
    p.own(g[0], [])
    c, rows = connect(e, p, d, d.bins)
    assert c.n_connected == len(d.bins)
    p.add(rows)
    e.dag_prune(2)
    for r in list(p.m.blocks):
        if r[1] == 1:
            del p.m.blocks[r]
    t = p.take()
    assert t.flags == M.PROPOSE_INCOMPLETE and t.taken == 14 and t.queue == 0
    assert r1[0] not in refs_of(t.includes)  # named by a block of round 3 (and of round 2)


def test_payloads_around_the_cut(store_engine, tag):
    """A payload entry as the last taken entry, directly before the cut, and one directly behind the
    cut's include, which stays -- with an include of a lower round behind the cut, which stays too. (The
    first entry left is always the include the cut stands on, or the queue is empty: core.rs:240-247.)"""
    e = store_engine
    g = [ref(a, 0) for a in range(1, 4)]
    x1, y1, w0, b2, c2 = ref(1, 1), ref(2, 1), ref(1, 0, 5), ref(1, 2), ref(2, 2)
    seeded(e, tag, [1] * 4, g + [x1, y1, w0, b2, c2])
    p = Pair(e, [1] * 4)
    p.add(g, in_order=True, tags=[1, 2, 3])
    p.own(ref(0, 0), [])
    p.add([], payload=501)  # a call of no rows: the payload entry alone
    p.add([x1], tags=[31])
    t = p.take()  # g1 g2 g3 P501 | x1
    assert (t.round, t.taken, t.next_entry, t.queue) == (1, 4, 31, 1) and t.payloads.tolist() == [501]
    assert refs_of(t.includes) == g
    p.own(ref(0, 1))
    p.add([], payload=502)
    p.add([w0], tags=[32])
    p.add([y1], tags=[33])
    p.add([b2], tags=[34], payload=503)
    assert p.m.round == 2
    t = p.take()  # x1 P502 w0 y1 | b2 P503
    assert (t.taken, t.next_entry, t.queue) == (4, 34, 2) and t.payloads.tolist() == [502]
    assert refs_of(t.includes) == [x1, w0, y1]
    p.own(ref(0, 2))
    p.add([w0, c2], tags=[35, 36])  # w0 again, of round 0, behind the entries that stayed
    assert p.m.round == 3
    t = p.take()  # b2 P503 w0 c2 |
    assert (t.taken, t.next_entry, t.queue) == (4, M.PROPOSE_NO_ENTRY, 0) and t.payloads.tolist() == [503]
    p.own(ref(0, 3))
    p.add([], payload=504)
    t = p.take()  # clock 3 <= own 3: nothing, whatever the queue holds
    assert (t.proposed, t.taken, t.next_entry, t.queue) == (0, 0, M.PROPOSE_NO_ENTRY, 1)


def test_one_include_record(store_engine, tag):
    """Stakes [7, 1, 1, 1]: seat 0 is a quorum alone, so a block with one include is valid; its record's
    list of length 1 (and one of length 2) goes through the stamping wave."""
    e = store_engine
    d = Dag(e, 4, [7, 1, 1, 1], distinct=False)
    a1, b1, c1, d1 = d.full()
    b2, c2 = d.layer([(1, [a1]), (2, [a1, b1])])
    ready(e, tag, d.pks, d.stakes, 4)
    e.index_insert_stored([ref(0, 2)])
    p = Pair(e, d.stakes)
    p.add(d.genesis[1:], in_order=True)
    p.own(d.genesis[0], [])
    c, rows = connect(e, p, d, d.bins)
    assert c.n_connected == 6 and [len(p.m.blocks[r]) for r in (b2, c2)] == [1, 2]
    p.add(rows + [ref(0, 2)])
    assert p.m.round == 3
    t = p.take()
    assert t.taken == 10 and refs_of(t.includes) == [c1, d1, b2, c2, ref(0, 2)] and t.flags == M.PROPOSE_INCOMPLETE


@pytest.fixture(scope="module")
def wide512(engine):
    """tests/wide_committee.py's 512-seat committee (thirteen heavy seats): every seat's block of round 1,
    and the heavy seats' blocks of round 2, each of which includes the whole round before (512 includes)."""
    import wide_committee as W

    plan = W.main_plan()
    d = W.new_dag(engine, plan)
    W.step(d, range(plan.n))
    W.step(d, plan.heavy)
    return d


def test_wide_round(store_engine, wide512, tag):
    """512 seats, one full round pending under blocks that each name all of it."""
    e, d = store_engine, wide512
    ready(e, tag, d.pks, d.stakes, 512)
    r3 = [ref(a, 3) for a in d.heavy]  # (references only: they move the clock past round 2)
    e.index_insert_stored(r3)
    p = Pair(e, list(d.stakes))
    p.add(d.genesis[1:], in_order=True)
    p.own(d.genesis[0], [])
    c, rows = connect(e, p, d, d.bins)
    assert c.n_connected == 512 + len(d.heavy)
    p.add(rows + r3, tags=list(range(len(rows) + len(r3))))
    assert p.m.round == 4
    t = p.take(cap=1 << 11)
    # every block of round 1 is named by a taken block of round 2: 6,656 stamps on 512 slots
    assert t.proposed == 1 and p.m.dropped >= 512 and d.rounds[2][0] in refs_of(t.includes)


# ---------------------------------------------------------------- the own block
@pytest.fixture(scope="module")
def own_dag(engine):
    """4 seats with stakes [2, 1, 1, 1], 6 full rounds; seat 0 is the validator and its stake is needed
    for every quorum of votes (the others hold 3 of 5; a quorum is above 3)."""
    d = Dag(engine, 4, [2, 1, 1, 1], distinct=False)
    for _ in range(6):
        d.full()
    return d


def others(d, rnd):
    return [d.blocks[r][0] for r in d.rounds[rnd] if r[0] != 0]


def walk(e, p, d, rounds, with_record=True, between=lambda step: None):
    """Seat 0's loop over Dag.full's rounds: take, own, then the other seats' blocks of that round."""
    for rnd in rounds:
        mine = d.first(rnd)[0]
        if with_record:
            t = p.take()
            between("take")
            # what the model chose is what Dag.full gave seat 0: the own last block, then the round before
            assert t.round == rnd and [p.m.own[0]] + refs_of(t.includes) == d.blocks[mine][1]
            before = e.dag_stats()
            p.own(mine)
            after = e.dag_stats()
            assert (after.records, after.includes) == (before.records + 1, before.includes + 4)
            assert e.index_lookup([mine]).tolist() == [M.REF_STORED]
            p.add(connect(e, p, d, others(d, rnd))[1], tags=[10 * rnd + k for k in range(3)], payload=rnd)
            between("add")
        else:
            e.index_insert_stored([mine])  # no record
            assert e.connect_blocks(others(d, rnd)).n_connected == 3
        assert e.connect_blocks([]).n_connected == 0


def test_own_record_closes_the_hole(store_engine, own_dag, tag):
    import linearize_model as L
    from test_gpu_linearize import check

    e, d = store_engine, own_dag
    leader = d.first(4)[1]
    for with_record in (False, True):
        ready(e, tag, d.pks, d.stakes, 4)
        p = Pair(e, d.stakes)
        p.add(d.genesis[1:], in_order=True)
        p.own(d.genesis[0], [])
        walk(e, p, d, range(1, 7), with_record)
        records = {r: list(i) for r, (_, i) in d.blocks.items() if with_record or r[0] != 0}
        dec = e.decide_leaders([(1, 1)])
        got = check(e, L.LevelRule(records), [leader])
        if with_record:
            assert got.status.tolist() == [M.LINEAR_OK] and dec.status.tolist() == [M.LEADER_COMMIT]
        else:
            assert got.status.tolist() == [M.LINEAR_INCOMPLETE] and dec.status.tolist() == [M.LEADER_UNDECIDED]


def test_rebuild_clear_and_refusals(own_dag, tag):
    d = own_dag
    e = M.Engine(devices=(0,))
    try:
        e.dag_reserve(4, 8)
        ready(e, tag, d.pks, d.stakes, 4)
        for call in (lambda: e.propose_add([ref(1, 0)]), lambda: e.propose_take(), lambda: e.propose_own(ref(0, 0), []),
                     lambda: e.propose_stats()):
            with pytest.raises(M.MvError) as err:
                call()
            assert err.value.code == M.E_INVALID_ARG
        p = Pair(e, d.stakes)
        with pytest.raises(M.MvError):
            e.propose_add([ref(1, 0, 77)])  # not in the index: the state stays
        p.check()
        with pytest.raises(M.MvError):
            e.propose_take()  # no own last block yet
        p.add(d.genesis[1:], in_order=True)
        p.own(d.genesis[0], [])
        with pytest.raises(M.MvError):
            e.propose_own(d.first(1)[1])  # another seat's
        with pytest.raises(M.MvError):
            e.propose_own(d.first(1)[0])  # no take outstanding
        p.check()
        serial = [0]

        def grow(step):
            """Enough inserts to grow the table: between take and own, and between add and take."""
            before = e.index_stats()
            k = before.capacity + 1
            e.index_insert([ref(5, 1000 + serial[0] + j, j) for j in range(k)], M.REF_WANTED)
            serial[0] += k
            assert e.index_stats().rebuilds > before.rebuilds

        walk(e, p, d, range(1, 4), between=grow)
        walk(e, p, d, range(4, 7))
        e.index_clear()
        assert e.propose_stats().words() == [0] * 8
    finally:
        e.close()


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("n", [4, 7])
def test_one_validators_view(store_engine, tag, n):
    """Seat 0 proposes from what the other seats deliver, in shuffled, delayed batches, for 30 rounds; the
    others include seat 0's block of the round before when there is one. Core is driven by the processed
    sets tests/connect_model.py gives, which the connected rows are held to on the way."""
    e = store_engine
    rng = random.Random(100 * n + tag)
    d = Dag(e, n, [1] * n, distinct=False)
    ready(e, tag, d.pks, d.stakes, n)
    model = CM.ThreeState(lambda img, offs, lens: [0] * len(offs), d.genesis)
    p = Pair(e, [1] * n)
    p.add(d.genesis[1:], in_order=True)
    p.own(d.genesis[0], [])
    seeds = np.frombuffer(b"".join(d.seeds), dtype=np.uint8).reshape(-1, 32)
    incs_of = {}
    own_at, pool, tagno, proposals = {0: d.genesis[0]}, [], [0], 0

    def processed(c, want, payload=None):
        rows = refs_of(c.connected[:, :6])
        assert rows == [r[0] for r in want.rows]
        for r in rows:
            p.m.blocks[r] = incs_of[r]
        dev = rng.random() < 0.5
        p.add(rows, tags=list(range(tagno[0], tagno[0] + len(rows))), payload=payload, dev=dev, stride=8 if dev else 6)
        tagno[0] += len(rows)

    for rnd in range(1, 31):
        prev = [r for r in d.rounds[rnd - 1] if r[0] != 0]
        mine = [own_at[rnd - 1]] if rnd - 1 in own_at else []
        for r in d.layer([(a, [x for x in prev if x[0] == a] + [x for x in prev if x[0] != a] + mine) for a in range(1, n)]):
            incs_of[r] = list(d.blocks[r][1])
            pool.append(d.blocks[r][0])
        rng.shuffle(pool)
        k = rng.randrange(0, len(pool) + 1) if rnd < 30 else len(pool)
        batch, pool = pool[:k], pool[k:]
        processed(e.connect_blocks(batch), model.connect(batch), payload=rnd)
        for _ in range(4):  # (a proposal can let the clock pass the next round too)
            t = p.take()
            if not t.proposed:
                break
            proposals += 1
            incs = [p.m.own[0]] + refs_of(t.includes)
            bn, _ = MB.encode(0, t.round, incs, [], [], t.round * 10**8, 0, bytes(64), bytes(32))
            buf = np.frombuffer(bn, dtype=np.uint8).copy()
            st, _, bd = e.seal_blocks(buf, [0], [len(bn)], seeds)
            assert st.tolist() == [M.SEAL_OK]
            mine = (0, t.round, bd[0].tobytes())
            incs_of[mine] = incs
            p.own(mine)
            own_at[t.round] = mine
            model.state[mine] = CM.STORED
            processed(e.connect_blocks([]), model.connect([]))
    assert proposals >= 10 and not pool
    top = e.dag_stats().highest_round
    com = e.commit_leaders([(r % n, r) for r in range(1, top - 1)])
    assert not any(int(f) & M.COMMIT_INCOMPLETE for f in com.flags)
