"""GPU: mv_wal_write / mv_dev_wal_write -- WalWriter::writev for many entries on the device
(wal.rs:150-188): positions, crc32 headers, zero gaps and bodies. The expected image is the oracle's
writer (oracle/wal.py, zlib.crc32: independent of the device's crc); every comparison is byte-exact.
Case lists: tests/wal_write_cases.py (tests/test_wal_write_cases.py shows they hit their edges)."""
import struct

import numpy as np
import pytest

import wal as OW
import wal_write_cases as C

pytestmark = pytest.mark.gpu

CANARY = 64


def write(engine, case, cap=None, prefill=0xA5, extra=CANARY):
    """One mv_wal_write into an array prefilled with `prefill`; cap defaults to the exact span."""
    img, pos, end = case.oracle()
    cap = len(img) if cap is None else cap
    out = np.full(cap + extra, prefill, dtype=np.uint8)
    got = engine.wal_write((np.frombuffer(case.buf, dtype=np.uint8), case.rows_array()), case.start, case.map_bits,
                           cap=cap, out=out)
    return got, out, (img, pos, end)


def assert_written(engine, case):
    """Image, positions and end against the oracle and wal_layout; nothing behind the span touched."""
    import mysticeti_amd as M

    got, out, (img, pos, end) = write(engine, case)
    assert got.end_pos == end and got.pos.tolist() == pos, case.name
    lay, lay_end = M.wal_layout(case.body_lens(), case.map_bits, case.start)
    assert got.pos.tolist() == lay.tolist() and got.end_pos == lay_end, case.name
    assert got.image.tobytes() == img, (case.name, first_diff(got.image.tobytes(), img))
    assert out[len(img):].tobytes() == b"\xa5" * CANARY, case.name


def first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def test_layout_edges(engine):
    for c in C.layout_edges():
        assert_written(engine, c)


@pytest.mark.parametrize("src_shift", range(8))
def test_crc_and_copy_alignment(engine, src_shift):
    for c in C.alignment(src_shift):
        assert_written(engine, c)


def test_own_blocks_at_every_alignment(engine):
    for c in C.own_alignment():
        assert_written(engine, c)


def test_not_a_byte_too_many(engine):
    import mysticeti_amd as M

    for c in C.layout_edges() + [C.append_case()]:
        # gaps come out zero whatever out held, and the canaries survive
        for fill in (0xA5, 0xFF):
            got, out, (img, pos, end) = write(engine, c, prefill=fill)
            assert got.image.tobytes() == img and out[len(img):].tobytes() == bytes([fill]) * CANARY, c.name
        if not img:
            continue
        # one byte short: no byte of out, the positions and the end as before
        got, out, _ = write(engine, c, cap=len(img) - 1)
        assert got.image.size == 0 and got.pos.tolist() == pos and got.end_pos == end, c.name
        assert out.tobytes() == b"\xa5" * (len(img) - 1 + CANARY), c.name
        # sizing only
        got = engine.wal_write((np.frombuffer(c.buf, dtype=np.uint8), c.rows_array()), c.start, c.map_bits, cap=0)
        assert got.pos.tolist() == pos and got.end_pos == end, c.name
    for c in C.refused():
        out = np.full(1024, 0xA5, dtype=np.uint8)
        with pytest.raises(M.MvError) as ei:
            engine.wal_write((np.frombuffer(c.buf, dtype=np.uint8), c.rows_array()), c.start, c.map_bits, out=out)
        assert ei.value.code == M.E_INVALID_ARG, c.name
        assert out.tobytes() == b"\xa5" * 1024, c.name


def test_append(engine):
    c = C.append_case()
    img, pos, end = c.oracle()
    gaps = [i for i in range(1, c.n) if pos[i] != pos[i - 1] + 16 + c.body_lens()[i - 1]]
    k = gaps[1]  # entry k straddles: cut in front of it, behind it and one further on either side
    for cuts in ([k], [k + 1], [k - 1], [k, k + 1], [k - 1, k], [1, k + 1], [gaps[0], gaps[2]]):
        at, got_img, got_pos = c.start, b"", []
        for lo, hi in zip([0] + cuts, cuts + [c.n]):
            part = c.slice(lo, hi, at)
            got, _, _ = write(engine, part, cap=len(img))
            got_img += got.image.tobytes()
            got_pos += got.pos.tolist()
            at = got.end_pos
        assert (got_img, got_pos, at) == (img, pos, end), cuts


def test_entries_as_tuples(engine):
    """The (tag, bytes) / (3, next_entry, bytes) form of Engine.wal_write."""
    entries = [(1, b"block"), (3, 0x1122334455667788, b"own block"), (2, b""), (5, bytes(range(200)))]
    w = OW.WalWriter(8, bytes(100))
    pos = [w.write(1, b"block"), w.writev(3, [struct.pack("<Q", 0x1122334455667788), b"own block"]), w.write(2, b""),
           w.write(5, bytes(range(200)))]
    got = engine.wal_write(entries, start=100, map_bits=8)
    assert got.image.tobytes() == w.image()[100:] and got.pos.tolist() == pos and got.end_pos == w.pos
    got = engine.wal_write([], start=9, map_bits=8)
    assert got.image.size == 0 and got.pos.size == 0 and got.end_pos == 9


@pytest.fixture(scope="module")
def sealed_dag():
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    e = M.Engine(devices=(0,))
    n_auth, rounds = 4, 5
    seeds = [MB.authority_seed(a) for a in range(n_auth)]
    blocks = MB.build_rounds_sealed(e, rounds, n_auth, seeds, n_inc=3, n_vr=2, with_tx=True)
    pks, stakes = MB.committee(e, n_auth, distinct=True)
    e.set_committee(pks, stakes, 0)
    e.index_reserve(4096)
    e.dag_reserve(512, 4096)
    yield e, blocks, n_auth
    e.close()


def dag_entries(blocks, n_auth):
    """A WAL as the core writes one: blocks, now and then the own block (authority 0), payload, state
    and commit entries (their bytes are opaque to the replay)."""
    entries = []
    for i, b in enumerate(blocks):
        if i % n_auth == 0:
            entries.append((3, 1000 + i, b))
            entries.append((2, b"payload %d" % i))
        else:
            entries.append((1, b))
        if i % 7 == 6:
            entries.append((5, b"commit" * (i % 5)))
    entries.insert(len(entries) // 2, (4, b"state"))
    return entries


def test_round_trip_through_the_readers(sealed_dag):
    import mysticeti_amd as M

    e, blocks, n_auth = sealed_dag
    bits = 12
    entries = dag_entries(blocks, n_auth)
    w = OW.WalWriter(bits)
    for x in entries:
        w.writev(x[0], [struct.pack("<Q", x[1]), x[2]] if len(x) == 3 else [x[1]])
    got = e.wal_write(entries, 0, bits)
    assert got.image.tobytes() == w.image() and got.end_pos == w.pos
    assert any(p % (1 << bits) == 0 for p in got.pos.tolist()[1:]), "the image crosses a map"
    pos, tag, ln, st = e.wal_verify(got.image, got.end_pos, bits)
    assert pos.tolist() == got.pos.tolist() and (st == M.WAL_OK).all()
    assert tag.tolist() == [x[0] for x in entries]
    assert ln.tolist() == [len(x[-1]) + (8 if len(x) == 3 else 0) for x in entries]
    rep = e.wal_replay(got.image, got.end_pos, bits)
    blk = [i for i, x in enumerate(entries) if x[0] in (1, 3)]
    assert rep.count == len(entries) and rep.n_blocks == len(blk) and (rep.blk_status == 0).all()
    assert rep.rows[:, 0].tolist() == blk
    assert rep.rows[:, 1].tolist() == [int(got.pos[i]) + 16 + (8 if entries[i][0] == 3 else 0) for i in blk]
    assert rep.rows[:, 9].tolist() == [entries[i][1] if entries[i][0] == 3 else M.WAL_NONE for i in blk]
    # the committer's records: from the device-written image and from the oracle-written one
    seeded = []
    for image in (got.image, np.frombuffer(w.image(), dtype=np.uint8)):
        e.index_clear()
        e.dag_prune(1 << 40)
        rep2, sd = e.wal_recover(image, got.end_pos, bits)
        ds = e.dag_stats()
        seeded.append(((sd.rows, sd.records, sd.includes, sd.wanted, sd.misfits),
                       (ds.records, ds.includes, ds.lowest_round, ds.highest_round), rep2.rows.tolist(),
                       rep2.summary.tolist(), rep2.last_seen.tolist()))
    assert seeded[0] == seeded[1] and seeded[0][0][0] == len(blk) and seeded[0][0][1] == len(blk)


def test_device_buffers(sealed_dag):
    """mv_dev_wal_write reads encoded and sealed blocks where mv_dev_encode_blocks left them (its
    offsets and lengths go into the rows as they are), writes what the host call writes, and
    mv_dev_wal_replay reads the image back."""
    import torch

    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    e, blocks, n_auth = sealed_dag
    dev = torch.device("cuda:0")

    def t64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)

    rounds = len(blocks) // n_auth
    heads, includes, payloads = MB.encoded_inputs(rounds, n_auth, 3, 2, True)
    seeds = np.frombuffer(b"".join(MB.authority_seed(a) for a in range(n_auth)), dtype=np.uint8).reshape(n_auth, 32)
    pbuf, poff, plen = (np.ascontiguousarray(x) for x in payloads)
    n = heads.shape[0]
    cap = sum((len(b) + 7) & ~7 for b in blocks)
    d_pay = torch.zeros(pbuf.shape[0] + 16, dtype=torch.uint8, device=dev)
    d_pay[:pbuf.shape[0]] = torch.from_numpy(pbuf.copy()).to(dev)
    d_img = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_off, d_len = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    d_st, d_sst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    total = e.dev_encode_blocks(0, t64(heads), t64(includes), d_pay, pbuf.shape[0], t64(poff), t64(plen), d_img, cap,
                                d_off, d_len, d_st, seal=True, link=True, d_seeds=torch.from_numpy(seeds.copy()).to(dev),
                                d_seal_status=d_sst)
    torch.cuda.synchronize()
    assert total == cap and not d_st.any() and not d_sst.any()
    img = d_img[:cap].cpu().numpy()
    offs, lens = d_off.cpu().numpy().view(np.uint64), d_len.cpu().numpy().view(np.uint64)
    assert [img[o:o + l].tobytes() for o, l in zip(offs.tolist(), lens.tolist())] == blocks
    # the rows, built on the device: authority 0's blocks are own blocks
    d_rows = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    d_rows[:, 0] = 1
    d_rows[::n_auth, 0] = 3
    d_rows[:, 1], d_rows[:, 2] = d_off, d_len
    d_rows[:, 3] = torch.arange(n, device=dev) + 500
    rows = d_rows.cpu().numpy().view(np.uint64)
    bits = 12
    for start in (0, 4093):
        host = e.wal_write((img, rows), start, bits)
        span = host.end_pos - start
        assert span > (2 << bits), "the image crosses maps"
        d_out = torch.full((span + CANARY + 16,), 0xA5, dtype=torch.uint8, device=dev)
        d_pos = torch.zeros(n, dtype=torch.int64, device=dev)
        # a cap one byte short: the positions and the end, no byte
        assert e.dev_wal_write(0, d_img, cap, d_rows, start, bits, d_out, span - 1, d_pos) == host.end_pos
        torch.cuda.synchronize()
        assert bool((d_out == 0xA5).all()) and d_pos.cpu().numpy().view(np.uint64).tolist() == host.pos.tolist()
        d_pos.zero_()
        assert e.dev_wal_write(0, d_img, cap, d_rows, start, bits, d_out, span, d_pos) == host.end_pos
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert got[:span].tobytes() == host.image.tobytes() and (got[span:] == 0xA5).all()
        assert d_pos.cpu().numpy().view(np.uint64).tolist() == host.pos.tolist()
        if start:
            continue
        # written from position 0 the bytes are a WAL image: mv_dev_wal_replay reads them back in place
        d_out[span:] = 0
        cnt = n + 8
        d_epos = torch.zeros(cnt, dtype=torch.int64, device=dev)
        d_tag, d_elen = torch.zeros(cnt, dtype=torch.int32, device=dev), torch.zeros(cnt, dtype=torch.int32, device=dev)
        d_est = torch.zeros(cnt, dtype=torch.uint8, device=dev)
        d_brows, d_bst = torch.zeros((cnt, 10), dtype=torch.int64, device=dev), torch.zeros(cnt, dtype=torch.uint8, device=dev)
        d_sum, d_seen = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(n_auth, dtype=torch.int64, device=dev)
        n_ent, n_blk = e.dev_wal_replay(0, d_out, span, span, bits, d_epos, d_tag, d_elen, d_est, d_brows, d_bst, d_sum,
                                        d_seen)
        assert (n_ent, n_blk) == (n, n)
        assert d_epos[:n].cpu().numpy().view(np.uint64).tolist() == host.pos.tolist()
        assert not d_est[:n].any() and not d_bst[:n].any()
        br = d_brows[:n].cpu().numpy().view(np.uint64)
        assert br[:, 2].tolist() == lens.tolist() and br[:, 4].tolist() == [1 + i // n_auth for i in range(n)]
        assert br[:, 9].tolist() == [500 + i if i % n_auth == 0 else M.WAL_NONE for i in range(n)]


def test_production_size(engine):
    """map_bits 24, a few thousand config-4-shape blocks: about 40 MB across two map boundaries."""
    import mysticeti_amd.blocks as MB

    base = MB.config4(engine, rounds=1, n_auth=100)  # 100 blocks of ~9.5 KB; the entries share their bytes
    buf, off, ln = MB.pack(base)
    n = 4300
    rows = np.zeros((n, 4), dtype=np.uint64)
    idx = np.arange(n) % len(base)
    rows[:, 0] = np.where(np.arange(n) % 128 == 5, 3, 1)
    rows[:, 1], rows[:, 2], rows[:, 3] = off[idx], ln[idx], np.arange(n)
    case = C.Case("production", 24, 0, buf.tobytes(), rows.tolist())
    img, pos, end = case.oracle()
    assert end > 2 << 24 and sum(1 for p in pos if p % (1 << 24) == 0) == 3
    got = engine.wal_write((buf, rows), 0, 24)
    assert got.end_pos == end and got.pos.tolist() == pos
    assert got.image.tobytes() == img
