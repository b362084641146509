"""GPU: the include checks and the threshold clock (types.rs:349-362, threshold_clock.rs:12-35,
committee.rs:50-57,121-127) on every form that restates them -- the host codec, the one-lane and
the wave ingest, the one-pass walk in both its bitmap widths, the comb kernels of the online
service and of the submission queue, and the frames path -- against the independent model of
tests/quorum_model.py, at the committee's edges: stakes past 2^32 and up to a total just under
2^63, 1 to 512 keys, duplicates, 64-bit rounds and authorities, first failures past the 64th
include. test_quorum_model.py holds the model and the C oracle to each other on the same cases.
Every status must equal the model's and both digests the oracle's."""
import numpy as np
import pytest

import frames_model as FM
import mysticeti_amd as M
import oracle as O
import quorum_model as Q

pytestmark = pytest.mark.gpu

SHORT = 8192  # blocks up to here fit the online service's window with room to spare


class Committee:
    def __init__(self, name):
        self.name = name
        stakes = Q.COMMITTEES[name]
        n = len(stakes)
        self.pks = np.frombuffer(b"".join(Q.committee_keys(n)), dtype=np.uint8).reshape(-1, 32)
        self.stakes = np.array(stakes, dtype=np.uint64)
        assert [int(s) for s in self.stakes] == stakes
        self.cases = Q.quorum_cases(n, stakes)  # signed once per committee
        self.bins = [c.bincode for c in self.cases]
        self.md, self.bd = [], []
        for c in self.cases:
            st, md, bd = O.block_verify(c.bincode, self.pks, self.stakes, 0)
            assert st == c.status, c.note  # (test_quorum_model.py's check)
            self.md.append(md)
            self.bd.append(bd)

    def load(self, eng):
        eng.set_committee(self.pks, self.stakes, 0)

    def check(self, idx, st, md, bd, what):
        assert len(st) == len(idx)
        for j, i in enumerate(idx):
            c = self.cases[i]
            assert int(st[j]) == c.status, (f"{self.name}, {what}: case {i} at {j} ({c.note}): "
                                            f"{M.BLOCK_STATUS[int(st[j])]}, the model says {Q.NAMES[c.status]}")
            assert md[j].tobytes() == self.md[i] and bd[j].tobytes() == self.bd[i], \
                f"{self.name}, {what}: case {i} at {j} ({c.note}): digest"


@pytest.fixture(scope="module", params=list(Q.COMMITTEES))
def com(request):
    return Committee(request.param)


@pytest.fixture(params=["in_comb", "two_kernel", "separate_hash", "batch_walk", "batch_stage"])
def ingest_form(request, opts):
    """The device ingest forms of test_gpu_ingest.py: on small calls the parse and the digests
    inside k_verify_comb16 (the default), k_block_ingest + the digests inside k_verify_comb16
    (MV_INGEST_IN_COMB=0) and k_block_ingest + a separate k_b2_quad launch (MV_HASH_IN_COMB=0);
    at batch size the one-pass walk (k_block_walk<4> up to 128 keys, k_block_walk<16> above; the
    default) and the staged form (k_block_ingest + k_b2_lane, MV_BLK_WALK=0)."""
    opts("MV_HASH_IN_COMB", request.param != "separate_hash")
    opts("MV_INGEST_IN_COMB", request.param != "two_kernel")
    opts("MV_BLK_WALK", request.param != "batch_stage")
    return request.param


@pytest.fixture(scope="module")
def host_engine():
    with M.Engine(devices=(0,), host_parse=True) as e:
        yield e


def batch_order(com):
    """Every case once, then the shorter half of them over and over up to MV_BATCH_MIN blocks: one
    batch-path call that stays a few MB even where a quorum takes 342 includes."""
    n = len(com.bins)
    idx = list(range(n))
    small = sorted(range(n), key=lambda i: (len(com.bins[i]), i))[:(n + 1) // 2]
    k = 0
    while len(idx) < M.BATCH_MIN:
        idx.append(small[k % len(small)])
        k += 1
    return idx


def test_device_forms(engine, com, ingest_form):
    com.load(engine)
    if ingest_form.startswith("batch"):
        idx = batch_order(com)
        b0 = engine.batch_stats()[0]
        st, md, bd = engine.verify_blocks([com.bins[i] for i in idx])
        com.check(idx, st, md, bd, ingest_form)
        assert engine.batch_stats()[0] > b0  # the call took the batch path
    else:
        idx = list(range(len(com.bins)))
        st, md, bd = engine.verify_blocks(com.bins)
        com.check(idx, st, md, bd, ingest_form)


def test_host_codec(host_engine, com):
    com.load(host_engine)
    st, md, bd = host_engine.verify_blocks(com.bins)
    com.check(range(len(com.bins)), st, md, bd, "host codec")


@pytest.mark.parametrize("per_call", [1, 64])
def test_online_service(engine, com, per_call):
    """Calls of short blocks must take the resident service; a block past its window goes alone
    and may go elsewhere: its verdict is held to the model all the same."""
    com.load(engine)
    short = [i for i in range(len(com.bins)) if len(com.bins[i]) <= SHORT]
    calls, cur, size = [], [], 0
    for i in short:  # up to per_call blocks and 96 KB per call
        if cur and (len(cur) == per_call or size + len(com.bins[i]) > 96 * 1024):
            calls.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += len(com.bins[i])
    calls.append(cur)
    o0 = engine.online_stats()[0]
    for idx in calls:
        st, md, bd = engine.verify_blocks([com.bins[i] for i in idx])
        com.check(idx, st, md, bd, f"online, {per_call} per call")
    assert engine.online_stats()[0] - o0 == len(calls)  # every call took the resident service
    for i in range(len(com.bins)):
        if len(com.bins[i]) > SHORT:
            st, md, bd = engine.verify_blocks([com.bins[i]])
            com.check([i], st, md, bd, "a long block alone")


def test_submission_queue(com):
    with M.Engine(devices=(0,), online=False) as eng:
        com.load(eng)
        st, md, bd = eng.verify_blocks(com.bins)
        com.check(range(len(com.bins)), st, md, bd, "queue")
        for i in range(0, len(com.bins), 7):  # and one block per call
            st, md, bd = eng.verify_blocks([com.bins[i]])
            com.check([i], st, md, bd, "queue, one per call")
        assert eng.online_stats()[0] == 0


def test_frames_path(engine, com):
    """One stream, every case in a Blocks frame of its own: the per-block statuses."""
    com.load(engine)
    stream = b"".join(FM.frame(FM.blocks_msg(FM.TAG_BLOCKS, [b])) for b in com.bins)
    buf = np.frombuffer(stream, dtype=np.uint8)
    soff, slen = np.array([0], np.uint64), np.array([len(stream)], np.uint64)
    got = engine.verify_frames_messages(buf, soff, slen)
    assert len(got.blk_off) == len(com.bins) and np.array_equal(got.blk_len, [len(b) for b in com.bins])
    for i, c in enumerate(com.cases):
        assert int(got.blk_status[i]) == c.status, (f"{com.name}, frames: case {i} ({c.note}): "
                                                    f"{M.BLOCK_STATUS[int(got.blk_status[i])]}, the model says "
                                                    f"{Q.NAMES[c.status]}")
    FM.assert_same(got, FM.model(buf, soff, slen, (com.pks, com.stakes, 0)))
    first_bad = next(i for i, c in enumerate(com.cases) if c.status != Q.OK)
    assert int(got.drop_msg[0]) == first_bad and got.bad_status[first_bad] == com.cases[first_bad].status


def test_overflowing_stakes_are_refused(engine):
    """committee.rs:50-57: the total is a checked sum, the threshold 2 * total / 3. A total, or
    twice a total, that wraps is refused, and the committee in force stays."""
    stakes = Q.COMMITTEES["n5_2p60"]
    assert 2**63 - 200 < sum(stakes) < 2**63
    c = Committee("n5_2p60")
    c.load(engine)  # twice the total just fits
    ok = [i for i, x in enumerate(c.cases) if x.status == Q.OK][:1] + \
         [i for i, x in enumerate(c.cases) if x.status == Q.THRESHOLD_CLOCK][:1]
    for bad in ([2**63, 2**63], [2**62] * 4, [2**64 - 1, 1], [2**63, 1]):
        pks = np.frombuffer(b"".join(Q.committee_keys(len(bad))), dtype=np.uint8).reshape(-1, 32)
        with pytest.raises(OverflowError):
            Q.quorum_threshold(bad)
        with pytest.raises(M.MvError, match="stake"):
            engine.set_committee(pks, np.array(bad, dtype=np.uint64), 0)
        st, md, bd = engine.verify_blocks([c.bins[i] for i in ok])
        c.check(ok, st, md, bd, f"after the refused stakes {bad}")
    top = [2**63 - 1]  # the largest total whose double fits
    engine.set_committee(c.pks[:1], np.array(top, dtype=np.uint64), 0)
    assert Q.quorum_threshold(top) == (2**64 - 2) // 3
