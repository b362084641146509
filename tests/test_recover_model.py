"""CPU: the model the GPU tests of mv_wal_recover compare against (tests/recover_model.py) on hand-
written images with the expected records written out here. Images come from oracle/wal.py's WalWriter;
the blocks of the first four cases are stand-ins -- a 56-byte reference, an include list, then the
MV_BLOCK_* the stand-in verdict reports -- and the rows come from tests/replay_model.py. The last
case writes the signed 48-block DAG of tests/test_index_model.py in the connected-row order of
tests/connect_model.py and asks for the connect path's own record list."""
import random
import struct

import numpy as np

import blocks as B
import commit_model as C
import connect_model as CM
import index_model as IM
import oracle as O
import recover_model as RC
import replay_model as RM
import wal as W
from test_index_model import N_AUTH, bad_signature, dag  # noqa: F401  (the fixture, the same 48 blocks)


def ref(a, r, fill):
    return (a, r, bytes([fill]) * 32)


def fake(own, incs=(), status=0):
    body = struct.pack("<Q", len(incs)) + b"".join(struct.pack("<QQQ", i[0], i[1], 32) + i[2] for i in incs)
    return struct.pack("<QQQ", own[0], own[1], 32) + own[2] + body + bytes([status]) + b"tail"


def stand_in(img, offs, lens):
    out = []
    for o, l in zip(offs.tolist(), lens.tolist()):
        k = struct.unpack_from("<Q", img, o + 56)[0] if l >= 64 else 0
        if l < 64 or struct.unpack_from("<Q", img, o + 16)[0] != 32 or 64 + 56 * k >= l:
            out.append(O.BLOCK_PARSE_ERROR)
        else:
            out.append(int(img[o + 64 + 56 * k]))
    return np.array(out, dtype=np.uint8)


def replayed(blocks, bits=12):
    """The blocks as a WAL (a 0..7-byte tag-2 entry ahead of each, every fourth an own block) and its rows."""
    w = W.WalWriter(bits)
    for k, b in enumerate(blocks):
        w.write(2, bytes([k & 255]) * (k % 8))
        w.write(3 if k % 4 == 3 else 1, (struct.pack("<Q", k) if k % 4 == 3 else b"") + b)
    res = RM.model(w.image(), w.pos, bits, N_AUTH, stand_in)
    assert res.n_blocks == len(blocks) and (res.status == RM.OK).all()
    return w.image(), res


G = [ref(a, 0, 0xA0 + a) for a in range(4)]
R1 = [ref(a, 1, 0x10 + a) for a in range(4)]
R2 = [ref(a, 2, 0x20 + a) for a in range(4)]
R3 = [ref(a, 3, 0x30 + a) for a in range(4)]


def layers():
    return ([fake(g, status=O.BLOCK_GENESIS) for g in G] + [fake(r, G) for r in R1] + [fake(r, R1) for r in R2] +
            [fake(r, R2[:3] + R1[3:]) for r in R3])


def test_whole_wal():
    img, res = replayed(layers())
    s = RC.Store()
    assert s.seed(img, res.rows, res.blk_status) == [16, 12, 48, 0, 0]
    assert [r for r, _ in s.records] == R1 + R2 + R3  # genesis rows are STORED without a record
    assert s.records[0][1] == G and s.records[11][1] == R2[:3] + R1[3:]
    assert s.stored() == set(G + R1 + R2 + R3) and s.wanted() == set() and s.stats() == (12, 48, 1, 3)
    # blocks start at every offset mod 8, own blocks 8 further on
    assert set((res.rows[:, 1] % 8).tolist()) == set(range(8))


def test_a_duplicate_reference():
    blocks = layers()
    blocks.insert(9, blocks[5])  # (1, 1) again, after round 2 began
    blocks.append(blocks[5])
    img, res = replayed(blocks)
    s = RC.Store()
    assert s.seed(img, res.rows, res.blk_status) == [18, 12, 48, 0, 0]
    assert [r for r, _ in s.records] == R1 + R2 + R3
    # ... and a reference that has a record already gets no second one
    assert s.seed(img, res.rows, res.blk_status) == [18, 0, 0, 0, 0] and len(s.records) == 12


def test_a_rejected_block_in_the_middle():
    blocks = layers()
    blocks[9] = fake(R2[1], R1, status=O.BLOCK_SIG_INVALID)
    img, res = replayed(blocks)
    s = RC.Store()
    assert s.seed(img, res.rows, res.blk_status) == [16, 11, 44, 0, 0]
    assert [r for r, _ in s.records] == R1 + [R2[0]] + R2[2:] + R3
    # its reference is stored all the same, so the blocks that include it find an entry: nothing is wanted
    assert R2[1] in s.stored() and R2[1] in s.records[-1][1] and s.wanted() == set()


def test_a_floor_cuts_a_wave_in_two():
    img, res = replayed(layers())
    for floor, want in ((0, R1 + R2 + R3), (1, R1 + R2 + R3), (2, R2 + R3), (3, R3), (4, [])):
        s = RC.Store()
        got = s.seed(img, res.rows, res.blk_status, floor)
        assert [r for r, _ in s.records] == want and got == [16, len(want), 4 * len(want), 0, 0]
        assert s.stored() == set(G + R1 + R2 + R3)  # the references rise whatever the floor
        pruned = RC.Store()
        pruned.seed(img, res.rows, res.blk_status)
        pruned.prune(floor)
        assert pruned.records == s.records  # what mv_dag_prune(floor) would have left


def test_a_wal_whose_first_rounds_are_missing():
    img, res = replayed(layers()[8:])  # rounds 2 and 3 alone
    s = RC.Store()
    assert s.seed(img, res.rows, res.blk_status) == [8, 8, 32, 4, 0]
    assert s.wanted() == set(R1) and [r for r, _ in s.records] == R2 + R3
    # the includes of round 3 that are rows of the call are not wanted, wherever the rows stand
    img, res = replayed(layers()[12:] + layers()[8:12])
    s = RC.Store()
    assert s.seed(img, res.rows, res.blk_status) == [8, 8, 32, 4, 0]
    assert s.wanted() == set(R1) and [r for r, _ in s.records] == R3 + R2


def test_a_row_that_does_not_fit_the_image():
    img, res = replayed(layers())
    rows = res.rows.copy()
    rows[5, 2] = 64 + 56 * 4 - 1  # an OK row whose length no longer holds its four includes
    rows[6, 2] = 63
    rows[7, 1] = len(img) - 10
    s = RC.Store()
    assert s.seed(img, rows, res.blk_status) == [16, 9, 36, 0, 3]
    assert [r for r, _ in s.records] == [R1[0]] + R2 + R3 and s.stored() == set(G + R1 + R2 + R3)


def test_connected_row_order_gives_the_connect_paths_records(dag):  # noqa: F811
    bins, genesis, verdicts = dag
    order = list(range(len(bins)))
    random.Random(5).shuffle(order)
    bad = bad_signature(bins[17])
    three = CM.ThreeState(verdicts, genesis)
    rows = []
    for lo in range(0, len(order), 7):  # several calls: blocks are parked and released later
        call = [bins[i] for i in order[lo:lo + 7]] + ([bad] if lo == 14 else [])
        rows += [r[0] for r in three.connect(call).rows]
    by_ref = {IM.own_ref(b): b for b in bins}
    assert len(rows) == len(bins) and not three.pending
    connect_records = [(r, IM.includes(by_ref[r])) for r in rows]
    # the same blocks as a WAL in that order, genesis first
    w = W.WalWriter(12)
    for k, b in enumerate([B.genesis(a).bincode() for a in range(N_AUTH)] + [by_ref[r] for r in rows]):
        w.write(2, bytes(k % 8))
        w.write(1, b)
    res = RM.model(w.image(), w.pos, 12, N_AUTH, verdicts)
    assert res.blk_status.tolist() == [O.BLOCK_GENESIS] * N_AUTH + [O.BLOCK_OK] * len(bins)
    s = RC.Store()
    assert s.seed(w.image(), res.rows, res.blk_status) == [52, 48, 192, 0, 0]
    assert s.records == connect_records and s.stored() == three.stored() and s.wanted() == set()
    # ... and both feed the rule the same: every leader of rounds 1..10 commits
    stakes = [1] * N_AUTH
    a, b = s.rule(stakes), RC.Store(genesis)
    for r, i in connect_records:
        b.add_record(r, i)
    leaders = [(rnd % N_AUTH, rnd) for rnd in range(1, 13)]
    got, want = a.commit(leaders), b.rule(stakes).commit(leaders)
    assert got[1] == want[1] == 10 and [w.row.status for w in got[0]] == [C.COMMIT] * 10 + [C.UNDECIDED] * 2
    assert [w.row.words(*l) for w, l in zip(got[0], leaders)] == [w.row.words(*l) for w, l in zip(want[0], leaders)]
