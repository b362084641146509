"""GPU: every path that builds a block's signed pre-image P and hashes it twice -- B2(P) and
B2(P || sig), which share a prefix -- on the corpus of tests/preimage_edges.py: the end of P and of
P || sig on every residue mod 128 behind every statement kind, every piece kind straddling a
128-byte boundary, many blocks before the last one, bincode lengths at the ingest window's fit test
at every start alignment, and tampered variants at the residues where a schedule changes.

The paths: the small-call forms (parse and digests inside k_verify_comb16; k_block_ingest + the
digests inside it; k_block_ingest + k_b2_quad), the batch forms (k_block_walk; k_block_ingest +
k_b2_lane), the resident online service at 1, 3, 4 and 64 blocks per call, the host codec
(MV_FLAG_HOST_PARSE), mv_dev_verify_blocks on packed device bytes, mv_verify_frames and mv_wal_replay.

Expected statuses and digests are the C oracle's (which tests/test_preimage_edges.py holds to
hashlib over the Python builder's pre-image and to tests/golden/preimage_edges.json); no form is
compared with another. Every comparison is bit-exact."""
import struct

import numpy as np
import pytest

import frames_model as FM
import mysticeti_amd as M
import preimage_edges as PE
import replay_model as RM
import wal as W

pytestmark = pytest.mark.gpu

SMALL_FORMS = ("in_comb", "two_kernel", "separate_hash")
BATCH_FORMS = ("batch_walk", "batch_stage")


@pytest.fixture(scope="module")
def corp(golden):
    """The signed corpus and the oracle's results, built once; pinned by the golden file."""
    assert PE.golden_summary() == golden("preimage_edges.json")
    return PE.corpus()


@pytest.fixture
def eng(engine, corp):
    engine.set_committee(*PE.committee())
    return engine


@pytest.fixture(scope="module")
def host_engine(corp):
    with M.Engine(devices=(0,), host_parse=True) as e:
        e.set_committee(*PE.committee())
        yield e


def set_form(opts, form):
    """The switch settings of test_gpu_ingest.py's ingest_form."""
    opts("MV_HASH_IN_COMB", form != "separate_hash")
    opts("MV_INGEST_IN_COMB", form != "two_kernel")
    opts("MV_BLK_WALK", form != "batch_stage")


def want_of(cases):
    res = PE.oracle_results()
    st = np.array([res[c.name][0] for c in cases], dtype=np.uint8)
    md = np.frombuffer(b"".join(res[c.name][1] for c in cases), dtype=np.uint8).reshape(-1, 32)
    bd = np.frombuffer(b"".join(res[c.name][2] for c in cases), dtype=np.uint8).reshape(-1, 32)
    return st, md, bd


def check(cases, got, what):
    """The status of every block, and both digests of every block the oracle could parse."""
    st, md, bd = (np.asarray(x) for x in got)
    wst, wmd, wbd = want_of(cases)
    assert st.shape == wst.shape, (what, st.shape, wst.shape)
    bad = np.flatnonzero(st != wst)
    assert not len(bad), (what, "status", len(bad), [(cases[i].name, int(st[i]), int(wst[i])) for i in bad[:5]])
    parsed = wst != PE.PARSE_ERROR
    for name, g, w in (("message digest", md, wmd), ("block digest", bd, wbd)):
        bad = np.flatnonzero(parsed & (g != w).any(axis=1))
        assert not len(bad), (what, name, len(bad), [cases[i].name for i in bad[:8]])


def shuffled(cases, seed=11):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


def clean(corp):
    return [c for c in corp if c.family != "tampered"]


# ---- small calls through the submission queue ---------------------------------------------------
@pytest.mark.parametrize("form", SMALL_FORMS)
def test_small_call_forms(eng, corp, opts, form):
    """The whole corpus in one call below MV_BATCH_MIN, the online service off."""
    set_form(opts, form)
    opts("MV_ONLINE", 0)
    cases = list(corp)
    assert len(cases) < M.BATCH_MIN
    q0 = eng.queue_stats()[0]
    check(cases, eng.verify_blocks([c.bincode for c in cases]), form)
    assert eng.queue_stats()[0] == q0 + 1
    some = [c for c in cases if c.family in ("two_shares", "tampered")][::-1]  # a second, short call: other neighbours
    check(some, eng.verify_blocks([c.bincode for c in some]), form + ", short call")


# ---- batch-size calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["corpus_order", "shuffled"])
@pytest.mark.parametrize("form", BATCH_FORMS)
def test_batch_forms(eng, corp, opts, form, order):
    """The corpus three times over in one call (>= MV_BATCH_MIN, no multiple of 64): the clean
    families pass the combined equation without a fallback; with the tampered family mixed in, the
    SIG_INVALID blocks force exactly one. Shuffled, the 64 lanes of a workgroup walk blocks of
    unlike lengths."""
    set_form(opts, form)
    for cases, fallbacks in ((clean(corp), 0), (list(corp), 1)):
        cases = cases * 3
        if order == "shuffled":
            cases = shuffled(cases)
        assert len(cases) >= M.BATCH_MIN and len(cases) % 64 and len(cases) < 2 * M.BATCH_MIN
        b0, f0 = eng.batch_stats()
        got = eng.verify_blocks([c.bincode for c in cases])
        b1, f1 = eng.batch_stats()
        check(cases, got, f"{form}, {order}, {len(cases)} blocks")
        assert (b1 - b0, f1 - f0) == (1, fallbacks)


# ---- the resident online service ----------------------------------------------------------------
@pytest.mark.parametrize("per_call", [1, 3, 4, 64])
def test_online_service(eng, corp, per_call):
    """tail_sweep through k_online's job shapes: every L at 64 blocks per call, every 4th L at 1, 3
    and 4 per call; the service takes every call."""
    cases = [c for c in corp if c.family == "tail_sweep" and (per_call == 64 or c.L % 4 == 0)]
    assert eng.get_option("MV_ONLINE") == 1
    o0 = eng.online_stats()[0]
    st, md, bd = [], [], []
    calls = 0
    for k in range(0, len(cases), per_call):
        r = eng.verify_blocks([c.bincode for c in cases[k:k + per_call]])
        calls += 1
        for acc, x in zip((st, md, bd), r):
            acc.append(x)
    assert eng.online_stats()[0] - o0 == calls
    check(cases, (np.concatenate(st), np.concatenate(md), np.concatenate(bd)), f"online, {per_call} per call")


def test_online_service_takes_the_tampered_and_long_blocks(eng, corp):
    """The tampered family one per call and in one call, and the long_tail blocks (many common
    blocks before P's end) twelve per call, all below the service's size limits."""
    tampered = [c for c in corp if c.family == "tampered"]
    long_tail = [c for c in corp if c.family == "long_tail"]
    o0 = eng.online_stats()[0]
    one = [eng.verify_blocks([c.bincode]) for c in tampered]
    check(tampered, tuple(np.concatenate([r[k] for r in one]) for k in range(3)), "online, tampered one per call")
    check(tampered, eng.verify_blocks([c.bincode for c in tampered]), "online, tampered in one call")
    calls = len(tampered) + 1
    for k in range(0, len(long_tail), 12):
        part = long_tail[k:k + 12]
        assert sum((len(c.bincode) + 7) & ~7 for c in part) <= 128 << 10
        check(part, eng.verify_blocks([c.bincode for c in part]), "online, long_tail")
        calls += 1
    assert eng.online_stats()[0] - o0 == calls


# ---- the host codec -----------------------------------------------------------------------------
def test_host_parse_engine(host_engine, corp):
    cases = clean(corp)
    check(cases, host_engine.verify_blocks([c.bincode for c in cases]), "host_parse")


# ---- the ingest window's fit test ---------------------------------------------------------------
def pack_at(cases, alignments):
    """(bytes, offsets, lengths): the blocks one after another, block i at the next offset with
    off & 7 == alignments[i] (None: wherever the one before ends); 16 readable bytes after the last."""
    out, offs = bytearray(), []
    for c, d in zip(cases, alignments):
        if d is not None:
            out += b"\xee" * ((d - len(out)) % 8)
            assert len(out) & 7 == d
        offs.append(len(out))
        out += c.bincode
    total = len(out)
    out += b"\xee" * 16
    return np.frombuffer(bytes(out), dtype=np.uint8), np.array(offs, dtype=np.int64), \
        np.array([len(c.bincode) for c in cases], dtype=np.int64), total


@pytest.mark.parametrize("form", SMALL_FORMS + BATCH_FORMS)
def test_window_threshold_device_api(eng, corp, opts, form):
    """mv_dev_verify_blocks on packed device bytes: every window_fit block starts at the alignment
    d it was sized for, so (off & 7) + len + 16 is 10239, 10240 and 10241 for every d (the wave
    path up to 10240, the one-lane path above); in the batch forms padded with tail_sweep blocks,
    packed back to back, to MV_BATCH_MIN."""
    import torch

    set_form(opts, form)
    fit = [c for c in corp if c.family == "window_fit"]
    cases, align = list(fit), [c.d or 0 for c in fit]
    if form in BATCH_FORMS:
        sweep = [c for c in corp if c.family == "tail_sweep"]
        pad = (sweep * 4)[:M.BATCH_MIN + 37 - len(fit)]
        # the window cases spread among the padding, not all in the first workgroup
        step = len(pad) // len(fit)
        cases, align = [], []
        for i, c in enumerate(fit):
            cases += [c] + pad[i * step:(i + 1) * step]
            align += [c.d or 0] + [None] * step
        cases += pad[len(fit) * step:]
        align += [None] * (len(pad) - len(fit) * step)
        assert len(cases) == M.BATCH_MIN + 37
    raw, offs, lens, total = pack_at(cases, align)
    for c, o, d in zip(cases, offs, align):
        if c.family == "window_fit" and c.d is not None:
            assert (int(o) & 7) + len(c.bincode) + 16 == c.value
    assert int(offs[-1] + lens[-1]) == total == raw.size - 16
    n = len(cases)
    dev = torch.device("cuda", 0)
    d_buf = torch.from_numpy(raw.copy()).to(dev)
    assert d_buf.data_ptr() % 8 == 0
    d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_md = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_bd = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_verify_blocks(0, d_buf, total, d_off, d_len, d_st, d_md, d_bd)
    torch.cuda.synchronize()
    check(cases, (d_st.cpu().numpy(), d_md.cpu().numpy(), d_bd.cpu().numpy()), f"device api, {form}")


def test_window_threshold_host_api(eng, corp):
    """A call whose longest block has len + 32 <= 10240 goes to the online service, one byte more
    to the queue (the rule test_online_service_size_limits_and_garbage states); the results are the
    oracle's either way."""
    cases = [c for c in corp if c.family == "window_fit" and c.d is None]
    assert [c.value for c in cases] == list(PE.FIT_VALUES)
    for c in cases:
        o0, q0 = eng.online_stats()[0], eng.queue_stats()[0]
        check([c], eng.verify_blocks([c.bincode]), c.name)
        took = (eng.online_stats()[0] - o0, eng.queue_stats()[0] - q0)
        assert took == ((1, 0) if len(c.bincode) + 32 <= PE.WINDOW else (0, 1)), (c.name, took)


# ---- frames and WAL replay ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(corp):
    """tail_sweep at every 8th L, and the tampered family."""
    return [c for c in corp if (c.family == "tail_sweep" and c.L % 8 == 0) or c.family == "tampered"]


@pytest.mark.parametrize("reps", [1, 24])
def test_frames(eng, sample, reps):
    """The sample as Blocks / RequestBlocksResponse frames of 1..7 blocks in five connections, once
    below MV_BATCH_MIN and once above it: the per-block statuses are the oracle's, the message and
    connection verdicts the frames model's; mv_frame_blocks + mv_verify_blocks on one connection's
    bytes give the digests too."""
    cases = sample * reps
    assert (len(cases) >= M.BATCH_MIN) == (reps > 1)
    rng = np.random.default_rng(3)
    streams, owner = [b""] * 5, [[] for _ in range(5)]
    i = 0
    while i < len(cases):
        k, s = int(rng.integers(1, 8)), int(rng.integers(5))
        tag = FM.TAG_BLOCKS if rng.integers(2) else FM.TAG_RESPONSE
        streams[s] += FM.frame(FM.blocks_msg(tag, [c.bincode for c in cases[i:i + k]])) + (FM.ping() if k & 1 else b"")
        owner[s] += cases[i:i + k]
        i += k
    soff, slen, out = [], [], b""
    for s in streams:
        out += b"\xee" * 3
        soff.append(len(out))
        slen.append(len(s))
        out += s
    buf = np.frombuffer(out + b"\xee" * 3, dtype=np.uint8)
    soff, slen = np.array(soff, np.uint64), np.array(slen, np.uint64)
    want = FM.model(buf, soff, slen, PE.committee())
    in_order = [c for s in range(5) for c in owner[s]]
    assert want.blk_status.tolist() == want_of(in_order)[0].tolist()  # every block is listed, in stream order
    assert (want.status != FM.OK).any() and (want.status == FM.OK).any()
    b0 = eng.batch_counters()[0]
    got = eng.verify_frames_messages(buf, soff, slen)
    assert eng.batch_counters()[0] - b0 == (1 if reps > 1 else 0)
    FM.assert_same(got, want, f"frames x{reps}")
    st, md, bd, consumed = eng.verify_frames(streams[2])
    assert consumed == len(streams[2])
    check(owner[2], (st, md, bd), f"verify_frames x{reps}")


@pytest.mark.parametrize("reps", [1, 24])
def test_wal_replay(eng, sample, reps):
    """The sample as tag-1 and tag-3 entries of a WAL image, once below MV_BATCH_MIN and once above
    it. A block that does not decode ends the replay (block_store.rs:73-74), so the image holds the
    blocks that parse, rejected ones included, and ends with one cut block; the other cut blocks
    each end a short image of their own."""
    parse = [c for c in sample if c.status != PE.PARSE_ERROR] * reps
    cut = [c for c in sample if c.status == PE.PARSE_ERROR]
    assert len(cut) == len(PE.TAMPER_RESIDUES) and (len(parse) >= M.BATCH_MIN) == (reps > 1)
    verdicts = RM.oracle_verdicts(*PE.committee())

    def image(blocks):
        w = W.WalWriter(16)
        for k, c in enumerate(blocks):
            if k % 5 == 1:
                w.write(2, bytes([k & 0xFF]) * (k % 8))  # the next block starts at another offset mod 8
            if k % 9 == 4:
                w.write(3, struct.pack("<Q", 1000 + k) + c.bincode)
            else:
                w.write(1, c.bincode)
        return w

    w = image(parse + cut[:1])
    want = RM.model(w.image(), w.pos, 16, PE.N_AUTH, verdicts)
    assert want.n_blocks == len(parse) and want.status[-1] == RM.BLOCK_DECODE
    assert want.blk_status.tolist() == want_of(parse)[0].tolist()
    b0 = eng.batch_counters()[0]
    got = eng.wal_replay(w.image(), end_pos=w.pos, map_bits=16)
    assert eng.batch_counters()[0] - b0 == (1 if reps > 1 else 0)
    RM.assert_same(got, want, f"replay x{reps}")
    if reps == 1:
        for c in cut[1:]:
            w = image(parse[:3] + [c] + parse[3:5])
            want = RM.model(w.image(), w.pos, 16, PE.N_AUTH, verdicts)
            assert (want.n_blocks, want.status[-1]) == (3, RM.BLOCK_DECODE)
            RM.assert_same(eng.wal_replay(w.image(), end_pos=w.pos, map_bits=16), want, c.name)
