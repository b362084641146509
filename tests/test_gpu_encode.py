"""GPU: mv_encode_blocks / mv_dev_encode_blocks against the plain-Python model of tests/encode_model.py
on the case lists of tests/encode_cases.py, byte for byte with the padding and the guard bytes behind
the span; sealing in the same call against mv_seal_blocks, mv_verify_blocks and the existing
builders; the propose chain take -> encode -> seal -> own; the device-buffer form; the neighbours."""
import numpy as np
import pytest

import encode_cases as C
import encode_model as EM
import mysticeti_amd as M
import seal_model as S
from mysticeti_amd import blocks as BL

pytestmark = pytest.mark.gpu
GUARD = 0xA5
TAIL = 40  # guard bytes behind the span


def arrays(call):
    heads = np.array(call.heads, dtype=np.uint64).reshape(-1, 10)
    includes = np.array(call.includes, dtype=np.uint64).reshape(-1, 6)
    payloads = (np.frombuffer(bytes(call.pbuf), dtype=np.uint8), np.array(call.poff, dtype=np.uint64),
                np.array(call.plen, dtype=np.uint64))
    return heads, includes, payloads


def seed_rows(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(-1, 32)


def assert_model(engine, call, **kw):
    """The GPU's image (padding and guard bytes included), offsets, lengths and statuses are the model's."""
    want = call.model()
    assert want.status == call.want
    out = np.full(want.out_bytes + TAIL, GUARD, dtype=np.uint8)
    got = engine.encode_blocks(*arrays(call), out=out, **kw)
    assert got.status.tolist() == want.status and got.out_bytes == want.out_bytes
    assert got.offs.tolist() == want.offs and got.lens.tolist() == want.lens
    if not kw.get("seal"):
        bad = [i for i, (o, l) in enumerate(zip(want.offs, want.lens)) if out[o:o + l].tobytes() != bytes(want.buf[o:o + l])]
        assert not bad, f"{call.name}: blocks differ from the model: {bad[:8]}"
        assert out[:want.out_bytes].tobytes() == bytes(want.buf), "the padding"
    assert (out[want.out_bytes:] == GUARD).all()
    return got, want


def test_shapes_equal_the_model(engine):
    """1. Include counts around the wave width, payload counts around the LDS step and tile, every
    statement kind, every source alignment, every padding length, both sides of the wave / workgroup
    switch: byte for byte."""
    got, want = assert_model(engine, C.shapes())
    assert set(want.status) == {EM.OK}
    assert {C.WG_BYTES - 1, C.WG_BYTES, C.WG_BYTES + 1} <= set(want.lens)
    assert {l % 8 for l in want.lens} == set(range(8))


def test_refusals(engine):
    """2. Every refused block has length 0 and takes no space; its neighbours are the bytes of a call
    without it."""
    c = C.refusals()
    got, want = assert_model(engine, c)
    refused = {i for i, s in enumerate(want.status) if s != EM.OK}
    assert {want.status[i] for i in refused} == {EM.BAD_HEAD, EM.BAD_PAYLOAD} and len(refused) >= 60
    assert all(got.lens[i] == 0 and got.offs[i] == got.offs[i + 1] for i in refused)
    less, _ = assert_model(engine, c.without(refused))
    assert less.buf.tobytes() == got.buf.tobytes()
    assert less.offs.tolist() == [int(o) for i, o in enumerate(got.offs) if i not in refused]


def test_too_long(engine):
    """2. MV_ENCODE_TOO_LONG one unit either side of MV_ENCODE_MAX_LEN, by the payload and by the
    include count (its span inside m); the block of exactly the limit is the largest a workgroup writes."""
    got, want = assert_model(engine, C.too_long())
    assert got.lens[0] == M.ENCODE_MAX_LEN and got.status.tolist()[1:4] == [M.ENCODE_TOO_LONG, M.ENCODE_TOO_LONG,
                                                                            M.ENCODE_BAD_HEAD]


def test_cap(engine):
    """3. A cap 8 bytes under the total writes nothing and seals nothing; a cap equal to the total
    leaves the bytes behind it."""
    c = C.refusals()
    want = c.model()
    n = len(c.heads)
    seeds = seed_rows([BL.authority_seed(a) for a in range(4)])
    for seal in (False, True):
        out = np.full(want.out_bytes + TAIL, GUARD, dtype=np.uint8)
        got = engine.encode_blocks(*arrays(c), out=out, cap=want.out_bytes - 8, seal=seal, seeds=seeds)
        assert (out == GUARD).all()
        assert got.out_bytes == want.out_bytes and got.lens.tolist() == want.lens and got.offs.tolist() == want.offs
        assert got.status.tolist() == want.status
        if seal:
            assert got.seal_status.tolist() == [M.SEAL_PARSE_ERROR] * n
            assert not got.msg_digest.any() and not got.block_digest.any()
        got = engine.encode_blocks(*arrays(c), out=out, cap=want.out_bytes, seal=seal, seeds=seeds)
        assert (out[want.out_bytes:] == GUARD).all() and got.out_bytes == want.out_bytes
        if not seal:
            assert out[:want.out_bytes].tobytes() == bytes(want.buf)
    # cap 0 sizes
    got = engine.encode_blocks(*arrays(c), cap=0)
    assert got.out_bytes == want.out_bytes and got.lens.tolist() == want.lens


def committee_for(engine, n_auth, distinct):
    pk, stakes = BL.committee(engine, n_auth, distinct)
    engine.set_committee(pk, stakes, 0)


def sealing_call():
    """Blocks of 5 authorities over 2 rounds whose includes name genesis (round 1) and round 1 (round 2)."""
    c = C.Call("sealing")
    gen = BL.genesis_refs(5)
    pay = c.pay(EM.payload(C.every_kind()[:6]), align=3)
    for a in range(5):
        c.block(a, 1, [gen[a]] + [g for g in gen if g[0] != a][:3], pay, 1 if a % 2 else 0)
    for a in range(5):
        c.block(a, 2, [(a, 1, bytes(32))] + [(x, 1, bytes(32)) for x in range(5) if x != a][:3], pay, a % 2)
    return c, [BL.authority_seed(a) for a in range(5)]


@pytest.mark.parametrize("link", [False, True])
def test_seal_equals_seal_blocks_on_the_models_bytes(engine, link):
    """4. encode_blocks(seal=True) is seal_blocks on the model's bytes: bytes, statuses, both digests;
    what it sealed verifies."""
    c, seeds = sealing_call()
    got, want = assert_model(engine, c, seal=True, link=link, seeds=seed_rows(seeds))
    buf = np.frombuffer(bytearray(want.buf), dtype=np.uint8)
    st, md, bd = engine.seal_blocks(buf, np.array(want.offs, dtype=np.uint64), np.array(want.lens, dtype=np.uint64),
                                    seed_rows(seeds), link=link)
    assert got.buf[:want.out_bytes].tobytes() == buf.tobytes()
    assert got.seal_status.tolist() == st.tolist() == [M.SEAL_OK] * len(c.heads)
    assert np.array_equal(got.msg_digest, md) and np.array_equal(got.block_digest, bd)
    # linked or not, every sealed block verifies (verify reads an include's authority and round, not its digest)
    committee_for(engine, 5, True)
    blocks = [got.buf[o:o + l].tobytes() for o, l in zip(want.offs, want.lens)]
    assert engine.verify_blocks(blocks)[0].tolist() == [M.BLOCK_OK] * len(blocks)


@pytest.mark.parametrize("n_auth,rounds,n_inc,n_vr,tx", [(4, 3, 4, 0, False), (100, 2, 67, 66, True)],
                         ids=["4x3", "100x2"])
def test_linked_dag_equals_build_rounds_sealed(engine, n_auth, rounds, n_inc, n_vr, tx):
    """4. One encode_blocks(seal=True, link=True) call over blocks.encoded_inputs is
    build_rounds_sealed's DAG byte for byte, and build_rounds_encoded returns the same."""
    seeds = [BL.authority_seed(a) for a in range(n_auth)]
    want = BL.build_rounds_sealed(engine, rounds, n_auth, seeds, n_inc, n_vr, tx)
    heads, includes, payloads = BL.encoded_inputs(rounds, n_auth, n_inc, n_vr, tx)
    got = engine.encode_blocks(heads, includes, payloads, seal=True, link=True, seeds=seed_rows(seeds))
    assert not got.status.any() and not got.seal_status.any()
    assert [got.buf[o:o + l].tobytes() for o, l in zip(got.offs.tolist(), got.lens.tolist())] == want
    assert BL.build_rounds_encoded(engine, rounds, n_auth, seeds, n_inc, n_vr, tx) == want
    committee_for(engine, n_auth, True)
    assert engine.verify_blocks(want)[0].tolist() == [M.BLOCK_OK] * len(want)


def test_link_order_and_a_refused_block(engine):
    """4. Rounds out of order under LINK: MV_E_INVALID_ARG. A refused block in the middle of a linked
    call: the includes that name it keep their bytes."""
    c, seeds = sealing_call()
    swapped = C.Call("swapped")
    swapped.includes, swapped.pbuf, swapped.poff, swapped.plen = c.includes, c.pbuf, c.poff, c.plen
    swapped.heads = c.heads[5:] + c.heads[:5]
    out = np.full(1 << 14, GUARD, dtype=np.uint8)
    with pytest.raises(M.MvError) as ei:
        engine.encode_blocks(*arrays(swapped), out=out, seal=True, link=True, seeds=seed_rows(seeds))
    assert ei.value.code == M.E_INVALID_ARG and (out == GUARD).all()
    # block 2 (authority 2, round 1) refused: marker 2
    c.heads[2][5] = 2
    c.want[2] = EM.BAD_HEAD
    got, want = assert_model(engine, c, seal=True, link=True, seeds=seed_rows(seeds))
    assert got.seal_status.tolist() == [M.SEAL_OK] * 2 + [M.SEAL_PARSE_ERROR] + [M.SEAL_OK] * 7
    assert not got.msg_digest[2].any() and not got.block_digest[2].any()
    model = bytearray(want.buf)
    st, md, bd = S.seal(model, [o for i, o in enumerate(want.offs) if i != 2], [l for i, l in enumerate(want.lens) if i != 2],
                        seeds, link=True)
    assert got.buf[:want.out_bytes].tobytes() == bytes(model)
    named = [i for i in range(5, 10) if any(row[0] == 2 for row in c.includes[c.heads[i][6]:c.heads[i][6] + c.heads[i][7]])]
    assert named
    for i in named:
        p = S.parse(got.buf[want.offs[i]:want.offs[i] + want.lens[i]].tobytes())
        assert [got.buf[want.offs[i] + at:want.offs[i] + at + 32].tobytes() for a, _, at in p.includes if a == 2] == [bytes(32)]


def test_device_form_rounds_out_of_order(engine):
    """4. The device-buffer form under LINK with rounds out of order: MV_E_INVALID_ARG, and d_out holds
    the encoded blocks unsealed, as the header says."""
    import torch

    dev = torch.device("cuda:0")
    c, seeds = sealing_call()
    c.heads = c.heads[5:] + c.heads[:5]
    want = c.model()
    heads, includes, (pbuf, poff, plen) = arrays(c)

    def t64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)

    n, cap = len(c.heads), want.out_bytes
    d_pay = torch.zeros(pbuf.shape[0] + 16, dtype=torch.uint8, device=dev)
    d_pay[:pbuf.shape[0]] = torch.from_numpy(pbuf.copy()).to(dev)
    d_out = torch.full((cap + 16,), GUARD, dtype=torch.uint8, device=dev)
    d_off, d_len = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    d_st, d_sst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    d_seeds = torch.from_numpy(seed_rows(seeds).copy()).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(M.MvError) as ei:
        engine.dev_encode_blocks(0, t64(heads), t64(includes), d_pay, pbuf.shape[0], t64(poff), t64(plen), d_out, cap,
                                 d_off, d_len, d_st, seal=True, link=True, d_seeds=d_seeds, d_seal_status=d_sst)
    torch.cuda.synchronize()
    assert ei.value.code == M.E_INVALID_ARG
    assert d_out[:cap].cpu().numpy().tobytes() == bytes(want.buf) and (d_out[cap:].cpu().numpy() == GUARD).all()
    assert d_len.cpu().numpy().view(np.uint64).tolist() == want.lens and not d_st.any().item()


def chain(e, encode_first=None):
    """5. Seat 0 of 4: reserve, own genesis, connect and add one full round, take. Returns the take."""
    committee_for(e, 4, False)
    gen = BL.genesis_refs(4)
    assert e.index_insert_stored(gen).tolist() == [0] * 4
    e.propose_reserve(0, 8)
    e.propose_add(M.ref_words(gen[1:]), in_order=True)
    e.propose_own(gen[0], [])
    round1 = BL.build_rounds(e, 1, 4, [bytes(32)] * 4, n_inc=4, n_vr=0, with_tx=False)
    con = e.connect_blocks(round1[1:])
    assert con.n_connected == 3
    if encode_first is not None:
        encode_first()
    e.propose_add(con.connected[:con.n_connected], tags=[7, 8, 9], payload=41)
    return e.propose_take(), gen, round1


def test_propose_chain():
    """5. take -> encode with seal -> own: the block verifies, its first include is the own last block,
    propose_own(includes=None) accepts it, and its bytes are the model's under seal_model."""
    e = M.Engine(devices=(0,))
    try:
        e.dag_reserve(64, 256)
        t, gen, _ = chain(e)
        assert t.proposed == 1 and t.n_includes >= 3 and t.payloads[:t.n_payloads].tolist() == [41]
        c = C.Call("own block")
        c.includes = [EM.ref_words(gen[0])] + [[int(w) for w in row] for row in t.includes[:t.n_includes]]
        j = c.pay(EM.payload([("share", b"the payload of token 41")]), align=5)
        c.block(0, t.round, [], j, 1, time_ns=1_700_000_000_123_456_789, inc0=0, k=len(c.includes))
        got, want = assert_model(e, c, seal=True, seeds=np.zeros((4, 32), dtype=np.uint8))
        assert got.seal_status.tolist() == [M.SEAL_OK]
        block = got.buf[:want.lens[0]].tobytes()
        model = bytearray(want.buf)
        assert S.seal(model, want.offs, want.lens, [bytes(32)] * 4)[0] == [S.OK] and block == bytes(model[:want.lens[0]])
        st, _, bd = e.verify_blocks([block])
        assert st.tolist() == [M.BLOCK_OK] and bd[0].tobytes() == got.block_digest[0].tobytes() == block[24:56]
        p = S.parse(block)
        assert p.includes[0][:2] == (0, 0) and block[p.includes[0][2]:p.includes[0][2] + 32] == gen[0][2]
        clock = e.propose_own((0, t.round, block[24:56]))
        assert e.propose_stats().words()[4] == t.round and clock.round >= t.round
    finally:
        e.close()


def test_device_form_equals_the_host_form(engine):
    """6. mv_dev_encode_blocks on arrays in HBM gives the host call's image, offsets, lengths, statuses
    and seal results; once more with a payload buffer whose last payload ends on its last byte."""
    import torch

    dev = torch.device("cuda:0")

    def t64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)

    sealing, seeds = sealing_call()
    ends = C.Call("ends on the last byte")
    ends.block(1, 2, [C.ref(a, 1) for a in range(3)], ends.pay(EM.payload(C.every_kind()), align=6), 1)
    assert ends.poff[-1] + ends.plen[-1] == len(ends.pbuf) and len(ends.pbuf) % 8
    for call, seal in ((C.shapes(), False), (sealing, True), (ends, False)):
        heads, includes, (pbuf, poff, plen) = arrays(call)
        host = engine.encode_blocks(heads, includes, (pbuf, poff, plen), seal=seal, link=seal,
                                    seeds=seed_rows(seeds) if seal else None)
        n, cap = heads.shape[0], host.out_bytes
        d_pay = torch.zeros(pbuf.shape[0] + 16, dtype=torch.uint8, device=dev)
        d_pay[:pbuf.shape[0]] = torch.from_numpy(pbuf.copy()).to(dev)
        d_out = torch.full((cap + 16,), GUARD, dtype=torch.uint8, device=dev)
        d_off, d_len = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        d_sst = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        d_md, d_bd = torch.zeros((n, 32), dtype=torch.uint8, device=dev), torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_seeds = torch.from_numpy(seed_rows(seeds).copy()).to(dev)
        torch.cuda.synchronize()
        total = engine.dev_encode_blocks(0, t64(heads), t64(includes), d_pay, pbuf.shape[0], t64(poff), t64(plen), d_out,
                                         cap, d_off, d_len, d_st, seal=seal, link=seal, d_seeds=d_seeds,
                                         d_seal_status=d_sst, d_md=d_md, d_bd=d_bd)
        torch.cuda.synchronize()
        assert total == cap, call.name
        assert d_out[:cap].cpu().numpy().tobytes() == host.buf[:cap].tobytes(), call.name
        assert (d_out[cap:].cpu().numpy() == GUARD).all()
        assert d_off.cpu().numpy().view(np.uint64).tolist() == host.offs.tolist()
        assert d_len.cpu().numpy().view(np.uint64).tolist() == host.lens.tolist()
        assert d_st.cpu().numpy().tolist() == host.status.tolist()
        if seal:
            assert d_sst.cpu().numpy().tolist() == host.seal_status.tolist()
            assert np.array_equal(d_md.cpu().numpy(), host.msg_digest) and np.array_equal(d_bd.cpu().numpy(), host.block_digest)


def test_neighbours():
    """7. A seal call, a take and a verify call give the same results and run the same stages in a
    context that encodes between them as in one that never does."""
    seen = []
    blocks = None
    for encodes in (False, True):
        e = M.Engine(devices=(0,))
        try:
            e.dag_reserve(64, 256)
            e.set_stage_timing(True)
            e.stage_times(reset=True)

            def encode():
                if encodes:
                    got = e.encode_blocks(*arrays(C.shapes()))
                    assert not got.status.any()
                    c, seeds = sealing_call()
                    assert not e.encode_blocks(*arrays(c), seal=True, link=True, seeds=seed_rows(seeds)).seal_status.any()

            encode()
            t, gen, round1 = chain(e, encode_first=encode)
            stripped = S.unseal(round1)
            raw, offs, lens = S.pack(stripped, fill=GUARD)
            buf = np.frombuffer(bytearray(raw), dtype=np.uint8)
            st, md, bd = e.seal_blocks(buf, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64),
                                       np.zeros((4, 32), dtype=np.uint8), link=True)
            encode()
            v = e.verify_blocks(round1)
            seen.append((t.includes[:t.n_includes].tobytes(), (t.proposed, t.round, t.taken, t.flags, t.next_entry, t.queue),
                         buf.tobytes(), st.tolist(), md.tobytes(), bd.tobytes(), v[0].tolist(), v[2].tobytes(),
                         e.stage_times(reset=True)[1]))
            blocks = round1
        finally:
            e.close()
    assert seen[0] == seen[1]
    assert seen[0][3] == [M.SEAL_OK] * 4 and seen[0][6] == [M.BLOCK_OK] * 4 and len(blocks) == 4
