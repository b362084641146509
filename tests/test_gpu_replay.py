"""GPU: mv_wal_replay / mv_dev_wal_replay -- the replay loop of BlockStore::open (block_store.rs:50-116)
on the device: the entry walk and crc check, the tag match, the decode and StatementBlock::verify
of every block entry in place in the image, the block rows, highest_round and
last_seen_by_authority -- against the plain-Python model of tests/replay_model.py with the CPU
oracle's block verdicts. Images come from oracle/wal.py's WalWriter, blocks and committee from
mysticeti_amd.blocks (config 1: 4 authorities). Every call goes through arrays pre-filled with a
sentinel, so each case also checks that nothing is written past the counts."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

import mysticeti_amd as M
import oracle as O
import replay_model as RM
import wal as W
from mysticeti_amd import blocks as MB

pytestmark = pytest.mark.gpu

N_AUTH = 4
S8, S32, S64 = 0xAB, 0xABABABAB, 0xABABABABABABABAB


@pytest.fixture(scope="module")
def corpus(engine):
    """64 signed config-1 blocks (16 rounds), the committee, and the oracle's verdict function."""
    bins = MB.config1(engine, 16)
    pks, stakes = MB.committee(engine, N_AUTH, distinct=False)
    assert len(bins) == 64
    return bins, (pks, stakes, 0), RM.oracle_verdicts(pks, stakes, 0)


@pytest.fixture(scope="module")
def with_statements(engine):
    """Four signed round-1 blocks of the same committee that carry a 512-byte Share and two VoteRanges."""
    return MB.build_rounds(engine, 1, N_AUTH, [bytes(32)] * N_AUTH, n_inc=4, n_vr=2, with_tx=True)


@pytest.fixture
def eng(engine, corpus):
    engine.set_committee(*corpus[1])
    return engine


def bad_signature(block: bytes) -> bytes:
    """One bit of the signature's s flipped and the digest recomputed over the new signature:
    parses, digest matches, signature invalid."""
    sig = bytearray(block[-64:])
    sig[40] ^= 0x10
    dig = hashlib.blake2b(M.block_preimage(block) + bytes(sig), digest_size=32).digest()
    return block[:24] + dig + block[56:-64] + bytes(sig)


def flip(block: bytes, at: int) -> bytes:
    return block[:at] + bytes([block[at] ^ 1]) + block[at + 1:]


def replay(e, image, end, bits, cap=None, cap_blocks=None, with_status=True):
    """mv_wal_replay through sentinel-filled arrays four places longer than the caps; checks the
    places past min(count, cap) / min(n_blocks, cap_blocks) and returns a WalReplay."""
    img = np.frombuffer(bytes(image), dtype=np.uint8)
    cap = img.size // 16 + 1 if cap is None else cap
    cap_blocks = img.size // 72 + 1 if cap_blocks is None else cap_blocks
    pos = np.full(cap + 4, S64, dtype=np.uint64)
    tag = np.full(cap + 4, S32, dtype=np.uint32)
    ln = np.full(cap + 4, S32, dtype=np.uint32)
    st = np.full(cap + 4, S8, dtype=np.uint8)
    rows = np.full((cap_blocks + 4, 10), S64, dtype=np.uint64)
    bst = np.full(cap_blocks + 4, S8, dtype=np.uint8)
    summary = np.full(3, S64, dtype=np.uint64)
    seen = np.full(N_AUTH + 2, S64, dtype=np.uint64)
    cnt, nb = ctypes.c_uint64(S64), ctypes.c_uint64(S64)
    rc = e.lib.mv_wal_replay(e.ctx, M._p(img) if img.size else None, img.size, end, bits, M._p(pos), M._p(tag), M._p(ln),
                             M._p(st), cap, ctypes.byref(cnt), M._p(rows), M._p(bst) if with_status else None, cap_blocks,
                             ctypes.byref(nb), M._p(summary), M._p(seen))
    assert rc == M.MV_OK, e.lib.mv_last_error(e.ctx)
    n, b = min(cnt.value, cap), min(nb.value, cap_blocks)
    assert (pos[n:] == S64).all() and (tag[n:] == S32).all() and (ln[n:] == S32).all() and (st[n:] == S8).all()
    assert (rows[b:] == S64).all() and (bst[b if with_status else 0:] == S8).all() and (seen[N_AUTH:] == S64).all()
    return M.WalReplay(pos[:n], tag[:n], ln[:n], st[:n], rows[:b], bst[:b], summary, seen[:N_AUTH], cnt.value, nb.value)


def check(e, w, verdicts, what, end=None, image=None):
    image = w.image() if image is None else image
    end = w.pos if end is None else end
    want = RM.model(image, end, w.map_bits, N_AUTH, verdicts)
    got = replay(e, image, end, w.map_bits)
    print(f"{what}: entries {got.count} last status {got.status[-1] if got.count else None}, rows {got.n_blocks} "
          f"by status {np.bincount(got.blk_status, minlength=1).tolist()}, summary {got.summary.tolist()}, "
          f"last_seen {got.last_seen.tolist()}")
    RM.assert_same(got, want, what)
    return got, want


def test_plain_replay(eng, corpus):
    """All five tags, own blocks, state entries before and after blocks, 4-KiB maps (padding), and a
    tag-2 entry of 0..7 bytes ahead of each block so that blocks start at every offset mod 8."""
    bins, _, verdicts = corpus
    w = W.WalWriter(12)
    w.write(4, b"state before")
    for k, b in enumerate(bins[:48]):
        w.write(2, bytes([k]) * (k % 8))
        if k % 5 == 2:
            w.write(3, struct.pack("<Q", 1000 + k) + b)
        else:
            w.write(1, b)
        if k % 7 == 3:
            w.write(5, b"commit" * 3)
        if k % 11 == 5:
            w.write(4, b"state %d" % k)
    w.write(4, b"state after")
    w.write(2, b"tail")
    got, want = check(eng, w, verdicts, "plain")
    # several maps, with padding where an entry would have straddled two
    assert w.pos > (4 << 12) and (got.pos[1:] != got.pos[:-1] + np.uint64(16) + got.len[:-1]).any()
    assert got.n_blocks == 48 and (got.status == M.WAL_OK).all() and (got.blk_status == M.BLOCK_OK).all()
    assert set((got.rows[:, 1] % 8).tolist()) == set(range(8))
    assert got.summary[0] == 12 and got.rows[int(got.summary[1]), 9] == 1047 and got.tag[int(got.summary[2])] == 4
    assert int(got.summary[2]) == got.count - 2 and got.last_seen.tolist() == [12, 12, 12, 12]
    own = got.rows[:, 9] != M.WAL_NONE
    assert got.tag[got.rows[own, 0].astype(np.int64)].tolist() == [3] * int(own.sum()) and own.sum() == 10
    # the same without the block status array
    nost = replay(eng, w.image(), w.pos, 12, with_status=False)
    assert np.array_equal(nost.rows, want.rows) and nost.summary.tolist() == want.summary.tolist()


def test_empty_and_tiny(eng, corpus):
    bins, _, verdicts = corpus
    got, _ = check(eng, W.WalWriter(12), verdicts, "size 0")
    assert (got.count, got.n_blocks) == (0, 0) and got.summary.tolist() == [0, M.WAL_NONE, M.WAL_NONE]
    assert got.last_seen.tolist() == [0] * N_AUTH
    w = W.WalWriter(12)
    w.write(2, b"only a payload")
    got, _ = check(eng, w, verdicts, "one entry, no block")
    assert (got.count, got.n_blocks) == (1, 0)
    w = W.WalWriter(12)
    w.write(1, bins[9])
    got, _ = check(eng, w, verdicts, "one block")
    assert (got.count, got.n_blocks) == (1, 1) and got.rows[0, :3].tolist() == [0, 16, len(bins[9])]
    # a block as the last entry of a map: it ends on the map's last byte
    w = W.WalWriter(12)
    w.write(2, bytes(4096 - 32 - len(bins[10])))
    p = w.write(1, bins[10])
    assert p + 16 + len(bins[10]) == 4096 == w.pos
    got, _ = check(eng, w, verdicts, "block ends its map (and the image)")
    assert got.n_blocks == 1 and got.blk_status.tolist() == [M.BLOCK_OK]
    w.write(4, b"next map")
    got, _ = check(eng, w, verdicts, "block ends its map")
    assert (got.count, got.n_blocks) == (3, 1) and got.pos[2] == 4096


def test_rejected_blocks_do_not_stop_the_replay(eng, corpus, with_statements):
    """One fault each: a tampered signature, a flipped digest byte, a flipped byte of a statement
    (the Share's bytes start 308 bytes in: reference 56, includes 8 + 4 x 56, count 8, tag and length 12)."""
    bins, com, verdicts = corpus
    assert O.block_verify(with_statements[2], *com)[0] == O.BLOCK_OK
    faulty = [bad_signature(bins[20]), flip(bins[21], 30), flip(with_statements[2], 308 + 100)]
    w = W.WalWriter(12)
    for k, b in enumerate(bins[16:20] + faulty + bins[23:26]):
        w.write(3 if k == 5 else 1, (struct.pack("<Q", 7) if k == 5 else b"") + b)
    w.write(4, b"state")
    got, want = check(eng, w, verdicts, "rejected blocks")
    assert got.count == 11 and got.n_blocks == 10 and (got.status == M.WAL_OK).all()
    assert got.blk_status[4] == M.BLOCK_SIG_INVALID and got.blk_status[5] == M.BLOCK_DIGEST_MISMATCH
    assert got.blk_status[6] not in (M.BLOCK_OK, M.BLOCK_PARSE_ERROR) and np.count_nonzero(got.blk_status) == 3
    offs, lens = got.rows[:, 1].copy(), got.rows[:, 2].copy()
    oracle = O.block_verify_batch(np.frombuffer(w.image() + b"\0", dtype=np.uint8), offs, lens, com[0], com[1], com[2])
    assert got.blk_status.tolist() == oracle[0].tolist()
    # the row carries the stored (claimed) digest, not the computed one
    assert got.digests[5].tobytes() == faulty[1][24:56] != oracle[2][5].tobytes()
    assert got.digests[3].tobytes() == oracle[2][3].tobytes()


def test_unknown_tag_and_authority_stop_it(eng, corpus):
    bins, _, verdicts = corpus
    for t in (0, 6, 0xFFFFFFFF):
        w = W.WalWriter(12)
        w.write(1, bins[0])
        w.write(t, b"what")
        w.write(1, bins[1])
        got, _ = check(eng, w, verdicts, f"tag {t}")
        assert (got.count, got.n_blocks, got.status[-1]) == (2, 1, M.WAL_UNKNOWN_TAG)
    # a block that parses, of authority = committee size (its digest and signature are not looked at)
    outsider = MB.encode(N_AUTH, 3, [], [], [], 0, 0, bytes(64), bytes(32))[0]
    assert O.block_verify(outsider, *corpus[1])[0] != O.BLOCK_PARSE_ERROR
    for tag, head in ((1, b""), (3, struct.pack("<Q", 9))):
        w = W.WalWriter(12)
        w.write(1, bins[0])
        w.write(1, bins[5])
        w.write(tag, head + outsider)
        w.write(1, bins[2])
        got, _ = check(eng, w, verdicts, f"outside authority, tag {tag}")
        assert (got.count, got.n_blocks, got.status[-1]) == (3, 2, M.WAL_UNKNOWN_AUTHORITY)
        assert got.last_seen.tolist() == [1, 2, 0, 0]


def test_cut_blocks_stop_it(eng, corpus):
    """A tag-1 payload that is a block cut at L bytes (its crc is right: the entry was written so),
    each in an image of its own; tag-3 payloads of 0..8 bytes; a tag-3 block cut after its reference."""
    bins, _, verdicts = corpus
    b = bins[33]
    cuts = sorted({0, 1, 55, 56, 57, len(b) - 1} | set(np.linspace(2, len(b) - 2, 30).astype(int).tolist()))
    assert len(cuts) >= 34
    payloads = [(1, b[:L]) for L in cuts] + [(3, bytes(range(n))) for n in range(9)]
    payloads += [(3, struct.pack("<Q", 5) + b[:56]), (3, struct.pack("<Q", 5) + b[:-1])]
    for tag, payload in payloads:
        w = W.WalWriter(12)
        w.write(1, bins[32])
        w.write(tag, payload)
        w.write(1, bins[34])
        got, _ = check(eng, w, verdicts, f"tag {tag}, payload of {len(payload)} bytes")
        assert (got.count, got.n_blocks, got.status[-1]) == (2, 1, M.WAL_BLOCK_DECODE)
        assert got.summary.tolist() == [9, M.WAL_NONE, M.WAL_NONE]


def test_the_earliest_failing_entry_wins(eng, corpus):
    bins, _, verdicts = corpus

    def image(bad_crc_at):
        w = W.WalWriter(12)
        pos = []
        for k in range(8):
            pos.append(w.write(2, b"payload %d" % k))
            pos.append(w.write(1, bins[k] if k != 3 else bins[k][:100]))  # entry 7 does not decode
        img = bytearray(w.image())
        img[pos[bad_crc_at] + 16 + 3] ^= 0x40
        return w, bytes(img)

    w, img = image(10)  # a crc failure after the decode failure
    got, _ = check(eng, w, verdicts, "crc failure after", image=img)
    assert (got.count, got.n_blocks, got.status[-1]) == (8, 3, M.WAL_BLOCK_DECODE)
    w, img = image(4)  # ... and one before it
    got, _ = check(eng, w, verdicts, "crc failure before", image=img)
    assert (got.count, got.n_blocks, got.status[-1]) == (5, 2, M.WAL_CRC_MISMATCH)
    # a file cut inside a block (the writer position past the end of the file)
    w = W.WalWriter(12)
    w.write(1, bins[0])
    w.write(1, bins[1])
    got, _ = check(eng, w, verdicts, "file cut inside a block", image=w.image()[:-7])
    assert (got.count, got.n_blocks, got.status[-1]) == (2, 1, M.WAL_CRC_MISMATCH)
    # ... whose missing tail is zeros, so that the crc still holds: no block is read past the image
    w = W.WalWriter(12)
    w.write(1, bins[0])
    w.write(1, bins[1] + bytes(20))
    got, _ = check(eng, w, verdicts, "file cut inside a block's zero tail", image=w.image()[:-7])
    assert (got.count, got.n_blocks, got.status[-1]) == (2, 1, M.WAL_BLOCK_DECODE)


def test_caps(eng, corpus):
    bins, _, verdicts = corpus
    w = W.WalWriter(12)
    for k in range(12):
        w.write(2, b"x" * k)
        w.write(1, bins[k])
    want = RM.model(w.image(), w.pos, 12, N_AUTH, verdicts)
    assert (want.count, want.n_blocks) == (24, 12)
    for cap, cap_blocks in ((5, 3), (0, 12), (24, 0), (0, 0), (23, 11)):
        got = replay(eng, w.image(), w.pos, 12, cap=cap, cap_blocks=cap_blocks)
        assert (got.count, got.n_blocks) == (24, 12), (cap, cap_blocks)
        assert got.pos.tolist() == want.pos[:cap].tolist() and got.status.tolist() == want.status[:cap].tolist()
        assert got.tag.tolist() == want.tag[:cap].tolist() and got.len.tolist() == want.len[:cap].tolist()
        assert np.array_equal(got.rows, want.rows[:cap_blocks]) and got.blk_status.tolist() == want.blk_status[:cap_blocks].tolist()
        assert got.summary.tolist() == want.summary.tolist() and got.last_seen.tolist() == want.last_seen.tolist()
    # the Python call with caps
    r = eng.wal_replay(w.image(), map_bits=12, cap=5, cap_blocks=3)
    assert (r.count, r.n_blocks, len(r.pos), r.rows.shape) == (24, 12, 5, (3, 10))
    RM.assert_same(eng.wal_replay(w.image(), map_bits=12), want, "Engine.wal_replay")


@pytest.fixture(scope="module")
def batch_case(corpus):
    """4,200 block entries: the 64 signed blocks repeated, one with a bad signature, some as own blocks."""
    bins, _, verdicts = corpus
    w = W.WalWriter(16)
    for i in range(4200):
        b = bad_signature(bins[2345 % 64]) if i == 2345 else bins[i % 64]
        if i % 97 == 0:
            w.write(3, struct.pack("<Q", i) + b)
        else:
            w.write(1, b)
    return w, RM.model(w.image(), w.pos, 16, N_AUTH, verdicts)


def test_batch_size_call_takes_the_walk_and_the_batch_equation(eng, batch_case):
    w, want = batch_case
    assert want.n_blocks == 4200 > M.BATCH_MIN
    before = eng.batch_counters()[0]
    got = replay(eng, w.image(), w.pos, 16)
    print(f"batch: batches {before} -> {eng.batch_counters()[0]}, statuses {np.bincount(got.blk_status).tolist()}")
    assert eng.batch_counters()[0] == before + 1  # one combined equation over the 4,200 blocks
    RM.assert_same(got, want, "batch")
    assert np.count_nonzero(got.blk_status) == 1 and got.blk_status[2345] == M.BLOCK_SIG_INVALID


def test_two_chunks_give_the_same_result(engine, corpus, batch_case):
    w, want = batch_case
    e = M.Engine(devices=(0,), max_batch=4096)
    try:
        e.set_committee(*corpus[1])
        before = e.batch_counters()[0]
        got = replay(e, w.image(), w.pos, 16)
        print(f"two chunks: batches {before} -> {e.batch_counters()[0]}")
        assert e.batch_counters()[0] == before + 1  # 4,096 blocks by the equation, 104 by the comb kernels
        RM.assert_same(got, want, "max_batch 4096")
    finally:
        e.close()


def test_device_call(eng, corpus):
    import torch

    bins, _, verdicts = corpus
    w = W.WalWriter(12)
    w.write(4, b"state")
    for k in range(20):
        w.write(2, b"y" * (k % 8))
        w.write(3 if k % 4 == 1 else 1, (struct.pack("<Q", k) if k % 4 == 1 else b"") + (bins[k] if k != 13 else bad_signature(bins[k])))
    img = np.frombuffer(w.image(), dtype=np.uint8)
    want = RM.model(w.image(), w.pos, 12, N_AUTH, verdicts)
    RM.assert_same(replay(eng, w.image(), w.pos, 12), want, "host call")
    dev = torch.device("cuda", 0)
    d_img = torch.zeros(img.size + 64, dtype=torch.uint8, device=dev)
    d_img[:img.size] = torch.from_numpy(img.copy()).to(dev)

    def outputs(cap, cap_b):
        return dict(d_pos=torch.full((cap,), -3, dtype=torch.int64, device=dev),
                    d_tag=torch.full((cap,), -3, dtype=torch.int32, device=dev),
                    d_len=torch.full((cap,), -3, dtype=torch.int32, device=dev),
                    d_status=torch.full((cap,), 255, dtype=torch.uint8, device=dev),
                    d_rows=torch.full((cap_b, 10), -3, dtype=torch.int64, device=dev),
                    d_blk_status=torch.full((cap_b,), 255, dtype=torch.uint8, device=dev),
                    d_summary=torch.full((3,), -3, dtype=torch.int64, device=dev),
                    d_last_seen=torch.full((N_AUTH,), -3, dtype=torch.int64, device=dev))

    o = outputs(want.count + 3, want.n_blocks + 3)
    torch.cuda.synchronize(dev)
    n, b = eng.dev_wal_replay(0, d_img, img.size, w.pos, 12, **o)
    print(f"device call: count {n}, n_blocks {b}")
    assert (n, b) == (want.count, want.n_blocks)
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    got = M.WalReplay(u64(o["d_pos"])[:n], o["d_tag"].cpu().numpy().view(np.uint32)[:n],
                      o["d_len"].cpu().numpy().view(np.uint32)[:n], o["d_status"].cpu().numpy()[:n], u64(o["d_rows"])[:b],
                      o["d_blk_status"].cpu().numpy()[:b], u64(o["d_summary"]), u64(o["d_last_seen"]), n, b)
    RM.assert_same(got, want, "device call")
    assert (o["d_status"].cpu().numpy()[n:] == 255).all() and (o["d_blk_status"].cpu().numpy()[b:] == 255).all()
    assert (o["d_pos"].cpu().numpy()[n:] == -3).all() and (o["d_rows"].cpu().numpy()[b:] == -3).all()
    # caps below the totals: the first entries and rows, the totals still returned
    o = outputs(4, 2)
    torch.cuda.synchronize(dev)
    assert eng.dev_wal_replay(0, d_img, img.size, w.pos, 12, **o) == (want.count, want.n_blocks)
    assert u64(o["d_pos"]).tolist() == want.pos[:4].tolist() and np.array_equal(u64(o["d_rows"]), want.rows[:2])
    assert u64(o["d_summary"]).tolist() == want.summary.tolist()
    # an image pointer off by 4
    with pytest.raises(M.MvError, match=r"\(-1\)"):
        eng.dev_wal_replay(0, d_img, img.size - 4, w.pos, 12, img_ptr=d_img.data_ptr() + 4, **o)


def test_no_committee_is_an_error(engine):
    e = M.Engine(devices=(0,))
    try:
        w = W.WalWriter(12)
        w.write(2, b"payload")
        with pytest.raises(M.MvError, match=r"\(-4\)"):
            e.wal_replay(w.image(), map_bits=12)
    finally:
        e.close()


def test_resources_return_after_destroy(engine, corpus):
    bins = corpus[0]
    before = engine.get_option("MV_LIVE_RESOURCES")
    e = M.Engine(devices=(0,))
    try:
        e.set_committee(*corpus[1])
        w = W.WalWriter(12)
        for k in range(6):
            w.write(3 if k == 2 else 1, (bytes(8) if k == 2 else b"") + bins[k])
        r = e.wal_replay(w.image(), map_bits=12)
        assert (r.count, r.n_blocks) == (6, 6) and engine.get_option("MV_LIVE_RESOURCES") > before
    finally:
        e.close()
    print(f"live resources: {before} -> {engine.get_option('MV_LIVE_RESOURCES')}")
    assert engine.get_option("MV_LIVE_RESOURCES") == before
