"""GPU: mv_verify_frames / mv_dev_verify_frames -- the received bytes of many connections walked
and verified on the device, one verdict per message and per connection (handle_read_stream and
the NetworkMessage decode, network.rs:400-457; process_blocks, net_sync.rs:314-383) -- against the
pure-Python model of tests/frames_model.py with the CPU oracle's block verdicts. Config-1
committee and blocks (tests/golden/blocks_config1.json)."""
import hashlib
import struct

import numpy as np
import pytest

import blocks as B
import frames_model as FM
import mysticeti_amd as M
import oracle as O
from frames_model import blocks_msg, frame, ping, refs_msg, subscribe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(golden):
    g = golden("blocks_config1.json")
    c = g["committee"]
    pks = np.frombuffer(b"".join(bytes.fromhex(x) for x in c["pks"]), dtype=np.uint8).reshape(-1, 32)
    bins = [b.bincode() for b in B.gen_config1(O.sign)]
    assert hashlib.sha256(b"".join(bins)).hexdigest() == g["sha256_bincode_concat"]
    return bins, (pks, np.array(c["stakes"], dtype=np.uint64), c["epoch"])


@pytest.fixture
def eng(engine, corpus):
    engine.set_committee(*corpus[1])
    return engine


def bad_signature(block: bytes) -> bytes:
    """The block with one bit of its signature's s flipped and its digest recomputed over the new
    signature: parses, digest matches, signature invalid."""
    sig = bytearray(block[-64:])
    sig[40] ^= 0x10
    dig = hashlib.blake2b(M.block_preimage(block) + bytes(sig), digest_size=32).digest()
    return block[:24] + dig + block[56:-64] + bytes(sig)


def unparsable(block: bytes) -> bytes:
    """The block with the digest-length word of its own reference set to 31."""
    return block[:16] + struct.pack("<Q", 31) + block[24:]


def show(what, got):
    """The figures of a result, printed before the assertions (visible with pytest -s)."""
    print(f"{what}: rows {got.rows.shape[0]} by status {np.bincount(got.status, minlength=6).tolist()}, "
          f"blocks {len(got.blk_off)} by status "
          f"{np.bincount(got.blk_status, minlength=1).tolist() if got.blk_status is not None else None}, "
          f"consumed {int(got.consumed.sum())}, streams dropped {int((got.drop_msg != M.MSG_NONE).sum())}")


def layout(streams, gap=0):
    """(buf, soff, slen) of the streams laid out one after another, `gap` bytes between them."""
    soff, slen, out = [], [], b""
    for s in streams:
        out += b"\xee" * gap
        soff.append(len(out))
        slen.append(len(s))
        out += s
    return np.frombuffer(out + b"\xee" * gap, dtype=np.uint8), np.array(soff, np.uint64), np.array(slen, np.uint64)


def framed(rng, blks, lo=1, hi=9, extras=True):
    """blks in Blocks / RequestBlocksResponse frames of lo..hi blocks, other messages and pings between."""
    out, i = b"", 0
    while i < len(blks):
        k = int(rng.integers(lo, hi + 1))
        out += frame(blocks_msg(FM.TAG_BLOCKS if rng.integers(2) else FM.TAG_RESPONSE, blks[i:i + k]))
        i += k
        if extras:
            out += [ping(), frame(subscribe(i)), frame(refs_msg(FM.TAG_REQUEST, int(rng.integers(0, 4)))),
                    frame(refs_msg(FM.TAG_NOT_FOUND, int(rng.integers(0, 4)))), b""][int(rng.integers(5))]
    return out


def test_plain_streams_in_pinned_memory(eng, corpus):
    """Five streams of ~40 blocks, in page-locked memory at odd offsets (the in-place DMA)."""
    bins, com = corpus
    rng = np.random.default_rng(1)
    streams = [framed(rng, bins[40 * s:40 * s + 38 + s]) for s in range(5)]
    buf, soff, slen = layout(streams, gap=13)
    arena = eng.host_empty((buf.size,))
    arena[:] = buf
    try:
        got = eng.verify_frames_messages(arena, soff, slen)
    finally:
        eng.host_free(arena)
    show("plain", got)
    assert (got.status == M.MSG_OK).all() and (got.drop_msg == M.MSG_NONE).all()
    assert np.array_equal(got.consumed, slen)
    for s in range(5):
        offs, lens, consumed = M.frame_blocks(streams[s])
        mine = np.flatnonzero(np.repeat(got.rows[:, 0], got.rows[:, 5]) == s)
        assert np.array_equal(got.blk_off[mine], offs + soff[s]) and np.array_equal(got.blk_len[mine], lens)
    assert np.array_equal(got.blk_status, eng.verify_blocks_packed(buf, got.blk_off, got.blk_len)[0])
    FM.assert_same(got, FM.model(buf, soff, slen, com))


@pytest.fixture(scope="module")
def verdict_case(corpus):
    bins, com = corpus
    rng = np.random.default_rng(2)
    good = lambda lo, n: frame(blocks_msg(FM.TAG_BLOCKS, bins[lo:lo + n]))
    m2 = bins[20:26]
    m2[3] = bad_signature(m2[3])
    a = good(0, 3) + ping() + good(3, 2) + frame(blocks_msg(FM.TAG_RESPONSE, m2)) + good(26, 4) + frame(subscribe())
    mb = bins[40:46]
    mb[1], mb[4] = bad_signature(mb[1]), unparsable(mb[4])
    b = good(30, 2) + frame(blocks_msg(FM.TAG_BLOCKS, mb)) + good(46, 1)
    c = good(50, 5) + frame(refs_msg(FM.TAG_REQUEST, 3)) + frame(struct.pack("<IQ", 5, 0)) + good(55, 2)
    d = framed(rng, bins[60:100])
    e = good(100, 4) + ping() + good(104, 6)[:-9]
    buf, soff, slen = layout([a, b, c, d, e], gap=5)
    return buf, soff, slen, FM.model(buf, soff, slen, com), [len(x) for x in (a, b, c, d, e)], len(good(100, 4)) + 12


def test_verdicts(eng, verdict_case):
    buf, soff, slen, want, lens, e_consumed = verdict_case
    got = eng.verify_frames_messages(buf, soff, slen)
    show("verdicts", got)
    rows = lambda s: np.flatnonzero(got.rows[:, 0] == s)
    # A: block 3 of message 2 has a bad signature
    ra = rows(0)
    assert got.status[ra].tolist() == [M.MSG_OK, M.MSG_OK, M.MSG_BLOCK_REJECTED, M.MSG_NOT_REACHED, M.MSG_NOT_REACHED]
    assert got.rows[ra[2], 7] == 3 and got.bad_status[ra[2]] == M.BLOCK_SIG_INVALID and got.drop_msg[0] == ra[2]
    # B: the unparsable block wins over the rejected one before it
    rb = rows(1)
    assert got.status[rb].tolist() == [M.MSG_OK, M.MSG_DECODE_ERROR, M.MSG_NOT_REACHED]
    assert got.rows[rb[1], 7] == 4 and got.bad_status[rb[1]] == M.BLOCK_PARSE_ERROR and got.drop_msg[1] == rb[1]
    # C: the walk stops at the tag-5 frame
    rc = rows(2)
    assert got.status[rc].tolist() == [M.MSG_OK, M.MSG_OK, M.MSG_DECODE_ERROR] and got.rows[rc[2], 1] == 5
    assert int(got.consumed[2]) < lens[2] and got.drop_msg[2] == rc[2]
    # D clean, E stops before its incomplete frame
    assert (got.status[rows(3)] == M.MSG_OK).all() and got.drop_msg[3] == M.MSG_NONE
    assert int(got.consumed[3]) == lens[3] and int(got.consumed[4]) == e_consumed and got.drop_msg[4] == M.MSG_NONE
    FM.assert_same(got, want)


def test_every_truncation_as_overlapping_streams(eng, corpus):
    bins, com = corpus
    whole = (frame(blocks_msg(FM.TAG_BLOCKS, bins[200:201])) + ping() + frame(refs_msg(FM.TAG_REQUEST, 2))
             + frame(blocks_msg(FM.TAG_RESPONSE, [bins[201]])) + frame(subscribe()))
    assert 900 < len(whole) < 1100
    buf = np.frombuffer(whole, dtype=np.uint8)
    slen = np.arange(len(whole) + 1, dtype=np.uint64)
    soff = np.zeros_like(slen)
    got = eng.verify_frames_messages(buf, soff, slen)
    show(f"truncations of {len(whole)} bytes", got)
    FM.assert_same(got, FM.model(buf, soff, slen, com))
    assert (got.status == M.MSG_OK).all()


def garbage_streams(bins):
    """2,000 streams of 64..600 bytes, half random bytes, half valid streams with 1..3 byte flips
    (seed fixed), and eight longer valid streams that carry a 51-reference RequestBlocks: that
    message needs 2,872 bytes, so no stream of at most 600 can ever be MV_MSG_TOO_MANY_REQUESTED."""
    rng = np.random.default_rng(2024)
    parts = [lambda: ping(), lambda: frame(subscribe(int(rng.integers(1 << 20)))),
             lambda: frame(blocks_msg(FM.TAG_BLOCKS, [bins[int(rng.integers(len(bins)))]])),
             lambda: frame(blocks_msg(FM.TAG_RESPONSE, [])),
             lambda: frame(refs_msg(FM.TAG_REQUEST, int(rng.integers(0, 4)))),
             lambda: frame(refs_msg(FM.TAG_NOT_FOUND, int(rng.integers(0, 4))))]

    def valid(lo, hi):
        while True:
            s, target = b"", int(rng.integers(lo, hi + 1))
            while len(s) < target:
                s += parts[int(rng.integers(len(parts)))]()
            if len(s) <= hi:
                return s

    def flipped(s):
        x = bytearray(s)
        for _ in range(int(rng.integers(1, 4))):
            x[int(rng.integers(len(x)))] = int(rng.integers(256))
        return bytes(x)

    out = []
    for k in range(2000):
        if k % 2:
            out.append(rng.integers(0, 256, size=int(rng.integers(64, 601)), dtype=np.uint8).tobytes())
        else:
            out.append(flipped(valid(64, 600)))
    for k in range(8):
        s = valid(64, 600) + frame(refs_msg(FM.TAG_REQUEST, 51)) + valid(64, 600)
        out.append(flipped(s) if k % 2 else s)
    return out


def test_garbage(eng, corpus):
    bins, com = corpus
    streams = garbage_streams(bins)
    assert all(64 <= len(s) <= 600 for s in streams[:2000])
    buf, soff, slen = layout(streams)
    want = FM.model(buf, soff, slen, com)
    assert set(want.status.tolist()) == set(range(6)), np.bincount(want.status, minlength=6)
    got = eng.verify_frames_messages(buf, soff, slen)  # (raises unless the call returns MV_OK)
    show("garbage (model)", want)
    show("garbage", got)
    FM.assert_same(got, want)


@pytest.fixture(scope="module")
def batch_case(corpus):
    bins, com = corpus
    assert len(bins) == 4096 == M.BATCH_MIN
    bins = list(bins)
    bins[2345] = bad_signature(bins[2345])
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, 4096), size=39, replace=False))
    streams = [framed(rng, bins[a:b], lo=20, hi=100, extras=False)
               for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [4096]]))]
    buf, soff, slen = layout(streams, gap=3)
    return buf, soff, slen, FM.model(buf, soff, slen, com)


def test_batch_size_call_takes_the_batch_path(eng, batch_case):
    buf, soff, slen, want = batch_case
    assert len(want.blk_off) == 4096 and len(soff) == 40
    before = eng.batch_counters()[0]
    got = eng.verify_frames_messages(buf, soff, slen)
    show(f"batch (batches {before} -> {eng.batch_counters()[0]})", got)
    assert eng.batch_counters()[0] == before + 1  # one combined equation over the 4,096 blocks
    FM.assert_same(got, want)
    assert np.count_nonzero(got.status == M.MSG_BLOCK_REJECTED) == 1
    assert np.count_nonzero(got.blk_status) == 1 and got.blk_status[2345] == M.BLOCK_SIG_INVALID


def test_device_variant_equals_the_host_call(eng, verdict_case):
    import torch

    buf, soff, slen, want = verdict_case[:4]
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(buf.size + 64, dtype=torch.uint8, device=dev)
    d_buf[:buf.size] = torch.from_numpy(buf.copy()).to(dev)
    d_soff = torch.from_numpy(soff.astype(np.int64)).to(dev)
    d_slen = torch.from_numpy(slen.astype(np.int64)).to(dev)
    ns, cap_m, cap_b = len(soff), want.rows.shape[0] + 3, len(want.blk_off) + 3
    d_cons = torch.zeros(ns, dtype=torch.int64, device=dev)
    d_drop = torch.zeros(ns, dtype=torch.int32, device=dev)
    d_rows = torch.zeros((cap_m, 8), dtype=torch.int32, device=dev)
    d_off = torch.zeros(cap_b, dtype=torch.int64, device=dev)
    d_len = torch.zeros(cap_b, dtype=torch.int64, device=dev)
    d_st = torch.full((cap_b,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    nm, nb = eng.dev_verify_frames(0, d_buf, buf.size, d_soff, d_slen, d_cons, d_drop, d_rows, d_off, d_len, d_st)
    print(f"device variant: n_msgs {nm}, n_blocks {nb}")
    assert (nm, nb) == (want.rows.shape[0], len(want.blk_off))
    got = M.FrameVerdicts(d_rows.cpu().numpy().view(np.uint32)[:nm], d_cons.cpu().numpy().view(np.uint64),
                          d_drop.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64)[:nb],
                          d_len.cpu().numpy().view(np.uint64)[:nb], d_st.cpu().numpy()[:nb])
    FM.assert_same(got, want)
    assert (d_st.cpu().numpy()[nb:] == 255).all()  # nothing written past the totals
    # caps below the totals: the first entries written, the totals still returned
    d_rows2 = torch.zeros((2, 8), dtype=torch.int32, device=dev)
    d_off2 = torch.zeros(5, dtype=torch.int64, device=dev)
    d_len2 = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert eng.dev_verify_frames(0, d_buf, buf.size, d_soff, d_slen, d_cons, d_drop, d_rows2, d_off2, d_len2) == (nm, nb)
    assert np.array_equal(d_rows2.cpu().numpy().view(np.uint32), want.rows[:2])
    assert np.array_equal(d_off2.cpu().numpy().view(np.uint64), want.blk_off[:5])


def test_two_logical_shards_give_the_result_of_one(engine, corpus, verdict_case, batch_case):
    e2 = M.Engine(devices=(0,), shards_per_device=2)
    try:
        e2.set_committee(*corpus[1])
        for what, case in (("verdicts", verdict_case), ("batch", batch_case)):
            buf, soff, slen, want = case[:4]
            cut = M.shard_plan(slen + np.uint64(64), 2)
            assert 0 < cut[1] < len(soff)  # both shards hold streams
            got = e2.verify_frames_messages(buf, soff, slen)
            show(f"two shards, {what}, cut {cut}", got)
            FM.assert_same(got, want, what)
    finally:
        e2.close()


def test_no_committee_is_an_error(engine):
    e = M.Engine(devices=(0,))
    try:
        with pytest.raises(M.MvError):
            e.verify_frames_messages(frame(subscribe()), [0], [16])
    finally:
        e.close()
