"""GPU: mv_seal_blocks / mv_dev_seal_blocks (StatementBlock::new_with_signer on bincode blocks with
placeholder digest and signature fields) against the existing builder, against mv_verify_blocks on
what it sealed, and against the plain-Python model of tests/seal_model.py at the length and link
edges. Every buffer carries guard bytes between and after its blocks, compared with the model's."""
import functools

import numpy as np
import pytest

import mysticeti_amd as M
import preimage_edges as PE
import seal_cases as C
import seal_model as S
from mysticeti_amd import blocks as BL

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def seed_rows(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(-1, 32)


def gpu_seal(engine, blocks, seeds, link, gaps=None):
    """Seals `blocks` packed with guard bytes: (the buffer, offs, lens, status, md, bd)."""
    raw, offs, lens = S.pack(blocks, gaps=gaps, fill=GUARD)
    buf = np.frombuffer(bytearray(raw), dtype=np.uint8)
    st, md, bd = engine.seal_blocks(buf, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64),
                                    seed_rows(seeds), link=link)
    return buf, offs, lens, st, md, bd


def assert_model(engine, blocks, seeds, link, gaps=None):
    """The GPU's buffer (guards included), statuses and digests are the model's."""
    buf, offs, lens, st, md, bd = gpu_seal(engine, blocks, seeds, link, gaps)
    want, _, _ = S.pack(blocks, gaps=gaps, fill=GUARD)
    wst, wmd, wbd = S.seal(want, offs, lens, seeds, link=link)
    assert st.tolist() == wst
    bad = [i for i in range(len(blocks)) if buf[offs[i]:offs[i] + lens[i]].tobytes() != bytes(want[offs[i]:offs[i] + lens[i]])]
    assert not bad, f"blocks differ from the model: {bad[:8]}"
    assert buf.tobytes() == bytes(want), "bytes outside the blocks changed"
    assert [x.tobytes() for x in md] == wmd and [x.tobytes() for x in bd] == wbd
    return buf, offs, lens, st, md, bd


@functools.lru_cache(maxsize=None)
def _corpora(engine):
    """[(name, the builder's blocks, seeds, committee is distinct)]: config 1 at 6 rounds and a
    100-authority config-4 DAG of 4 rounds, built once by the existing builder."""
    return (("config1", BL.config1(engine, 6), [bytes(32)] * 4, False),
            ("config4", BL.config4(engine, 4), [BL.authority_seed(a) for a in range(100)], True))


@pytest.fixture(scope="module", params=[0, 1], ids=["config1", "config4"])
def corpus(engine, request):
    return _corpora(engine)[request.param]


def committee_for(engine, n_auth, distinct):
    pk, stakes = BL.committee(engine, n_auth, distinct)
    engine.set_committee(pk, stakes, 0)


def test_equals_the_builder(engine, corpus):
    """1. The builder's DAG with own digests, signatures and in-corpus include digests zeroed, sealed
    with link=True, is the builder's output byte for byte; digests are mv_verify_blocks' on the original."""
    name, blocks, seeds, distinct = corpus
    stripped = S.unseal(blocks)
    assert sum(a != b for a, b in zip(stripped, blocks)) == len(blocks)
    gaps = [i % 8 for i in range(len(blocks))]
    buf, offs, lens, st, md, bd = gpu_seal(engine, stripped, seeds, True, gaps)
    assert st.tolist() == [M.SEAL_OK] * len(blocks)
    want, _, _ = S.pack(blocks, gaps=gaps, fill=GUARD)
    assert buf.tobytes() == bytes(want)
    committee_for(engine, len(seeds), distinct)
    vst, vmd, vbd = engine.verify_blocks(blocks)
    assert vst.tolist() == [M.BLOCK_OK] * len(blocks)
    assert np.array_equal(md, vmd) and np.array_equal(bd, vbd)
    # the Python entry that wraps it
    n_inc, n_vr, tx = (4, 0, False) if name == "config1" else (67, 66, True)
    rounds = len(blocks) // len(seeds)
    sealed = BL.build_rounds_sealed(engine, rounds, len(seeds), seeds, n_inc, n_vr, tx)
    if n_vr == 0:
        assert sealed == blocks
    else:  # its VoteRanges name genesis blocks (the link rule covers includes only): same sizes and verdicts
        assert [len(b) for b in sealed] == [len(b) for b in blocks] and sealed[:len(seeds)] == blocks[:len(seeds)]
        assert engine.verify_blocks(sealed)[0].tolist() == [M.BLOCK_OK] * len(blocks)


def test_round_trip_small_and_walk_paths(engine):
    """2. What the call sealed verifies: n = MV_BATCH_MIN (the walk / batch path) and one below it (the
    comb path), a 1024-level DAG."""
    n = M.BATCH_MIN
    blocks = BL.build_rounds_sealed(engine, n // 4, 4, [bytes(32)] * 4, n_inc=4, n_vr=0, with_tx=False)
    assert len(blocks) == n
    committee_for(engine, 4, False)
    buf, offs, lens = BL.pack(blocks)
    for m in (n, n - 1):
        st, md, bd = engine.verify_blocks_packed(buf, offs[:m], lens[:m])
        assert st.tolist() == [M.BLOCK_OK] * m
        assert all(bd[i].tobytes() == blocks[i][24:56] for i in (0, 5, m - 1))
    # the chain of levels against the model, where Python integers can follow: the last round's
    # digests depend on every round before it
    head = 24
    want, o, l = S.pack(S.unseal(blocks[:head]))
    S.seal(want, o, l, [bytes(32)] * 4, link=True)
    assert bytes(want[:o[-1] + l[-1]]) == b"".join(blocks[:head])


def test_length_edges(engine):
    """3. Every block of tests/preimage_edges.py -- |P| and |P| + 64 at 0 and +-1 around the 128-byte
    Blake2b block, the ingest window's fit test, tampered and cut blocks -- at the start alignment its
    case names, against the model. A valid block of the corpus was signed with the same seed, so sealing
    it again restores its own bytes."""
    cases = PE.corpus()
    blocks = [c.bincode for c in cases]
    seeds = [BL.authority_seed(a) for a in range(PE.N_AUTH)]
    gaps, pos = [], 0
    for i, c in enumerate(cases):  # block i starts at c.d mod 8 (window_fit), else at i mod 8
        d = c.d if c.d is not None else i % 8
        gaps.append((d - pos) % 8 + 8)
        pos += gaps[-1] + len(c.bincode)
    buf, offs, lens, st, md, bd = assert_model(engine, blocks, seeds, False, gaps)
    assert all(o % 8 == (c.d if c.d is not None else i % 8) for i, (o, c) in enumerate(zip(offs, cases)))
    want_st = [M.SEAL_PARSE_ERROR if c.status == PE.PARSE_ERROR else M.SEAL_OK for c in cases]
    assert st.tolist() == want_st
    for i, c in enumerate(cases):
        if c.status in (PE.OK, PE.GENESIS) and c.block is not None and any(c.block.signature):
            assert buf[offs[i]:offs[i] + lens[i]].tobytes() == c.bincode, c.name


def test_link_edges(engine):
    """4. The link rule's cases in one call, against the model; then rounds out of order, n = 0, n = 1."""
    blocks, want_status, _ = C.link_corpus()
    seeds = C.seeds()
    buf, offs, lens, st, md, bd = assert_model(engine, blocks, seeds, True, gaps=[3 + i for i in range(len(blocks))])
    assert [M.SEAL_STATUS[x] for x in st] == want_status
    # rounds out of order: MV_E_INVALID_ARG, the buffer unchanged; a parse error between them does not count
    swapped = [blocks[7], blocks[4], blocks[0]]
    raw, o, l = S.pack(swapped, fill=GUARD)
    b = np.frombuffer(bytearray(raw), dtype=np.uint8)
    with pytest.raises(M.MvError) as ei:
        engine.seal_blocks(b, o, l, seed_rows(seeds), link=True)
    assert ei.value.code == M.E_INVALID_ARG and b.tobytes() == bytes(raw)
    assert_model(engine, swapped, seeds, False)
    # n = 0 and n = 1
    g = np.frombuffer(bytearray(b"guard bytes"), dtype=np.uint8)
    st0, md0, bd0 = engine.seal_blocks(g, [], [], seed_rows(seeds), link=True)
    assert st0.shape == (0,) and g.tobytes() == b"guard bytes"
    for link in (False, True):
        assert_model(engine, blocks[:1], seeds, link, gaps=[5])
    # no seeds at all: every block that parses has an unknown author
    st, _, _ = engine.seal_blocks(np.frombuffer(bytearray(raw), dtype=np.uint8), o, l, np.zeros((0, 32), np.uint8))
    assert st.tolist() == [M.SEAL_UNKNOWN_AUTHOR, M.SEAL_PARSE_ERROR, M.SEAL_UNKNOWN_AUTHOR]


@pytest.mark.parametrize("link", [False, True])
def test_untouched_bytes(engine, link):
    """5. Blocks at byte offsets 0..7 mod 8 (tag-2 WAL entries shift them so), guard bytes between and
    after them: only the blocks change."""
    seeds = [BL.authority_seed(a) for a in range(8)]
    g = BL.genesis_refs(8)
    blocks = [C.blk(a, 1, [g[a]], n_extra=a) for a in range(8)] + \
             [C.blk(a, 2, [(x, 1, C.STALE) for x in range(8)], n_extra=3 * a) for a in range(8)]
    gaps, pos = [], 0
    for i, b in enumerate(blocks):
        gaps.append((i % 8 - pos) % 8 + 8 * (i % 3))
        pos += gaps[-1] + len(b)
    buf, offs, lens, st, md, bd = assert_model(engine, blocks, seeds, link, gaps)
    assert [o % 8 for o in offs] == [i % 8 for i in range(16)] and st.tolist() == [M.SEAL_OK] * 16
    inside = np.zeros(buf.shape[0], dtype=bool)
    for o, l in zip(offs, lens):
        inside[o:o + l] = True
    assert (buf[~inside] == GUARD).all() and (~inside).sum() >= 16


def test_neighbours(engine):
    """6. A verify call and a connect call before and after a seal call in one context give the
    verdicts and run the stages they do in a context that never seals."""
    name, blocks, seeds, distinct = _corpora(engine)[0]
    plain, sealing = M.Engine(devices=(0,)), M.Engine(devices=(0,))
    try:
        seen = []
        for e in (plain, sealing):
            committee_for(e, 4, False)
            e.set_stage_timing(True)
            e.stage_times(reset=True)
            assert e.index_insert_stored(M.ref_words(BL.genesis_refs(4))).tolist() == [0] * 4
            out = []
            for part in (blocks[:8], blocks[8:]):
                v = e.verify_blocks(part)
                c = e.connect_blocks(part)
                out.append((v[0].tolist(), v[2].tobytes(), c.blk_status.tolist(), c.blk_state.tolist(), c.n_connected,
                            c.connected.tobytes()))
                if e is sealing and part is blocks[:8]:
                    st = gpu_seal(e, S.unseal(blocks), seeds, True)[3]
                    assert st.tolist() == [M.SEAL_OK] * len(blocks)
            seen.append((out, e.stage_times(reset=True)[1], e.pending_stats().stored))
        assert seen[0] == seen[1]
        assert seen[0][0][1][0] == [M.BLOCK_OK] * (len(blocks) - 8) and seen[0][2] == 4 + len(blocks)
    finally:
        plain.close()
        sealing.close()


def test_device_variant(engine, corpus):
    """7. mv_dev_seal_blocks patches an image in HBM to what the host call returns; guards included."""
    import torch

    name, blocks, seeds, distinct = corpus
    stripped = S.unseal(blocks)
    gaps = [8 * (i % 2) + i % 8 for i in range(len(blocks))]
    buf, offs, lens, st, md, bd = gpu_seal(engine, stripped, seeds, True, gaps)
    raw, _, _ = S.pack(stripped, gaps=gaps, fill=GUARD)
    dev = torch.device("cuda:0")
    d_buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    d_len = torch.tensor(lens, dtype=torch.int64, device=dev)
    d_seeds = torch.from_numpy(seed_rows(seeds).copy()).to(dev)
    n = len(blocks)
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    d_md = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_bd = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.dev_seal_blocks(0, d_buf, len(raw) - 16, d_off, d_len, d_seeds, d_st, d_md, d_bd, link=True)
    assert d_buf.cpu().numpy().tobytes() == buf.tobytes()
    assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_md.cpu().numpy(), md)
    assert np.array_equal(d_bd.cpu().numpy(), bd)
    # without the digest arrays, unlinked: the host call's unlinked result
    hbuf, _, _, hst, _, _ = gpu_seal(engine, stripped, seeds, False, gaps)
    d_buf2 = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    engine.dev_seal_blocks(0, d_buf2, len(raw) - 16, d_off, d_len, d_seeds, d_st, link=False)
    assert d_buf2.cpu().numpy().tobytes() == hbuf.tobytes() and np.array_equal(d_st.cpu().numpy(), hst)


def test_seal_signs_as_ed25519_sign(engine):
    """8. Seal and sign share one signer: five blocks of seal_cases, one per authority; the 64
    signature bytes seal_blocks leaves in each block are ed25519_sign(seed[a], md[i])'s. The key rows
    (a mod l, prefix, public key) stay on the device, so their public keys are held to that call's pk
    through what they feed: the challenge H(R || A || m) inside the equal signature, which also
    verifies under pk."""
    seeds = C.seeds()
    g = BL.genesis_refs(C.N_AUTH)
    blocks = [C.blk(a, 1, [g[a]], n_extra=a) for a in range(C.N_AUTH)]
    buf, offs, lens, st, md, bd = gpu_seal(engine, blocks, seeds, False)
    assert st.tolist() == [M.SEAL_OK] * C.N_AUTH
    pk, sig = engine.ed25519_sign(seed_rows(seeds), md)
    for i in range(C.N_AUTH):
        assert buf[offs[i] + lens[i] - 64:offs[i] + lens[i]].tobytes() == sig[i].tobytes(), i
    assert engine.ed25519_verify(md, sig, pk=pk).tolist() == [M.SIG_OK] * C.N_AUTH
    assert len({p.tobytes() for p in pk}) == C.N_AUTH


@pytest.mark.parametrize("n", [64, M.BATCH_MIN])
def test_seal_stream_equals_the_hash_kernels(engine, n):
    """9. The seal stream and the hash kernels share one compression: over the tail_sweep family of
    tests/preimage_edges.py (|P| % 128 through every value, every tail kind), seal_blocks' md is
    Engine.blake2b256 of the model's pre-image and bd of pre-image || signature -- the four-lane hash
    at 64 strings, the one-lane hash at MV_BATCH_MIN."""
    sweep = PE.family("tail_sweep")
    if n < len(sweep):  # the tails in turn, |P| % 128 at the schedule's edges and at the even values between
        want = list(PE.RESIDUES) + [r for r in range(2, 127, 2) if r != 64][:n - len(PE.RESIDUES)]
        cases = [next(c for c in sweep if c.tail == PE.TAILS[i % 5] and len(c.block.preimage()) % 128 == r)
                 for i, r in enumerate(want)]
    else:
        cases = [sweep[i % len(sweep)] for i in range(n)]
    assert len(cases) == n and {c.tail for c in cases} == set(PE.TAILS)
    assert set(PE.RESIDUES) <= {len(c.block.preimage()) % 128 for c in cases}
    seeds = [BL.authority_seed(a) for a in range(PE.N_AUTH)]
    buf, offs, lens, st, md, bd = gpu_seal(engine, [c.bincode for c in cases], seeds, False)
    assert st.tolist() == [M.SEAL_OK] * n
    pre = [c.block.preimage() for c in cases]
    sigs = [buf[offs[i] + lens[i] - 64:offs[i] + lens[i]].tobytes() for i in range(n)]
    assert sigs == [c.block.signature for c in cases]
    assert [x.tobytes() for x in md] == engine.blake2b256(pre)
    assert [x.tobytes() for x in bd] == engine.blake2b256([p + s for p, s in zip(pre, sigs)])
