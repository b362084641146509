"""GPU: soundness of the batch path through the public calls.

Cancelling pairs: s_i + d and s_j - d (mod l). Each signature alone is rejected by single
verification, but their errors cancel in the combined equation whenever z_i = z_j, so a
coefficient that repeats per lane, wave, workgroup, chunk or copy chunk would accept both (a
consensus split: single verification rejects them). The equation must fail, and the fallback must
reject exactly the two rows.

Chosen s: under a small-order key A, [8][k]A = O for every k, so R = [s]B with any s < l is a valid
signature of any message. That gives full control of s in accepted signatures on every path that
consumes s digit by digit (the comb B-table recoding, sum z s and -[sum z s]B); the same rows with
one bit of s flipped must be rejected.
"""
import numpy as np
import pytest

import blocks as B
import mysticeti_amd as M
import oracle as O
import zip215 as Z

pytestmark = pytest.mark.gpu

N = 8192
DELTAS = [1, 1 << 125, Z.L - 1]
STARTS = [1, 64, 256, 1024, 2777]  # a lane, a wave, a workgroup and a chunk start; an interior index


def signed_rows(n, seed, n_keys=0):
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if not n_keys:
        pk, sig = O.sign_batch(rng.integers(0, 256, size=(n, 32), dtype=np.uint8), msg)
        return msg, sig, pk
    seeds = rng.integers(0, 256, size=(n_keys, 32), dtype=np.uint8)
    ki = rng.integers(0, n_keys, size=n).astype(np.uint32)
    ki[:n_keys] = np.arange(n_keys)
    pk, sig = O.sign_batch(seeds[ki], msg)
    return msg, sig, pk, ki, pk[:n_keys].copy()


def shift_s(sig, row, delta):
    s = (int.from_bytes(sig[row, 32:].tobytes(), "little") + delta) % Z.L
    sig[row, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)


def with_pair(sig, i, j, delta):
    out = sig.copy()
    shift_s(out, i, delta)
    shift_s(out, j, -delta)
    return out


def counters_delta(engine, fn):
    c0 = engine.batch_counters()
    out = fn()
    c1 = engine.batch_counters()
    return out, tuple(b - a for a, b in zip(c0, c1))


def expect_pair_rejected(st, msg, sig2, pk, i, j):
    """Statuses equal the oracle's (single verification is per row: the two changed rows are
    judged by it, every other row is a signed one): both rows 1, all others 0."""
    ref = np.zeros(len(st), np.uint8)
    ref[[i, j]] = O.verify_batch(pk[[i, j]], sig2[[i, j]], msg[[i, j]])
    assert list(ref[[i, j]]) == [1, 1]
    assert (st == ref).all(), np.nonzero(st != ref)[0][:8]


@pytest.fixture(scope="module")
def rows():
    msg, sig, pk = signed_rows(N, 101)
    assert (O.verify_batch(pk, sig, msg) == 0).all()
    return msg, sig, pk


@pytest.fixture
def one_group(engine):
    engine.set_batch_groups(1)  # one equation per batch, no adaptive guard or dense route
    yield engine
    engine.set_batch_groups(0)


@pytest.mark.parametrize("stride", [1, 64, 256, 1024, 4096])
def test_cancelling_pairs_fail_the_equation(one_group, rows, stride):
    engine = one_group
    msg, sig, pk = rows
    for i in STARTS:
        for delta in DELTAS:
            j = i + stride
            s2 = with_pair(sig, i, j, delta)
            st, d = counters_delta(engine, lambda: engine.ed25519_verify(msg, s2, pk))
            expect_pair_rejected(st, msg, s2, pk, i, j)
            assert d == (1, 1, 1, 1), (i, j, delta, d)  # the equation failed: not silently satisfied


def test_cancelling_pair_under_one_committee_key(one_group):
    """Both members signed by the same committee key: the pair's A terms land in one per-key sum
    (the aggregated A term)."""
    engine = one_group
    msg, sig, pk, ki, keys = signed_rows(N, 102, n_keys=7)
    engine.set_committee(keys, np.ones(7, np.uint64))
    same = np.nonzero(ki == 3)[0]
    for i, j, delta in [(int(same[5]), int(same[6]), 1), (int(same[0]), int(same[-1]), 1 << 125),
                        (int(same[10]), int(same[400]), Z.L - 1)]:
        s2 = with_pair(sig, i, j, delta)
        st, d = counters_delta(engine, lambda: engine.ed25519_verify(msg, s2, key_idx=ki))
        expect_pair_rejected(st, msg, s2, pk, i, j)
        assert d == (1, 1, 1, 1), (i, j, d)


@pytest.mark.parametrize("i,j,failing", [(3 * 1024 + 5, 3 * 1024 + 5 + 64, 1), (2 * 1024, 3 * 1024 - 1, 1),
                                         (1000, 1000 + 1024, 2), (0, N - 1, 2)])
def test_cancelling_pair_in_eight_groups(engine, rows, i, j, failing):
    """Eight sub-batch equations of 1024 signatures: a pair inside one group fails (and
    re-verifies) exactly that group, a pair split across two groups fails both."""
    msg, sig, pk = rows
    engine.set_batch_groups(8)
    try:
        s2 = with_pair(sig, i, j, 1 << 125)
        st, d = counters_delta(engine, lambda: engine.ed25519_verify(msg, s2, pk))
        expect_pair_rejected(st, msg, s2, pk, i, j)
        assert d == (1, 1, 8, failing)
    finally:
        engine.set_batch_groups(0)


def test_cancelling_pair_across_copy_chunks(one_group, opts):
    """Pinned inputs in 4096-signature copy chunks (k_bv_prep launched chunk by chunk, blk0 =
    chunk start / 256): a pair one chunk apart. The call runs as two batches (0.7 / 0.3 of it);
    the pair lies in the first, whose equation must fail."""
    engine = one_group
    opts("MV_STREAM_CHUNK_LOG2", 12)
    n = 9 * M.BATCH_MIN + 333
    msg, sig, pk = signed_rows(n, 103)
    pm, ps, pp = (engine.host_empty(a.shape, a.dtype) for a in (msg, sig, pk))
    try:
        pm[...], pp[...] = msg, pk
        for i, delta in [(4096, 1), (8192 + 5, 1 << 125), (3 * 4096 + 255, Z.L - 1)]:
            j = i + 4096
            s2 = with_pair(sig, i, j, delta)
            ps[...] = s2
            st, d = counters_delta(engine, lambda: engine.ed25519_verify(pm, ps, pp))
            expect_pair_rejected(st, msg, s2, pk, i, j)
            assert d == (2, 1, 2, 1), d
    finally:
        for a in (pm, ps, pp):
            engine.host_free(a)


def test_cancelling_pair_on_device_buffers(one_group, rows):
    import torch

    engine = one_group
    msg, sig, pk = rows
    i, j = 256, 256 + 1024
    s2 = with_pair(sig, i, j, 1)
    dev = torch.device("cuda", 0)
    dm, ds, dp = (torch.from_numpy(x.copy()).to(dev) for x in (msg, s2, pk))
    dst = torch.full((N,), 255, dtype=torch.uint8, device=dev)
    ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.dev_verify_batch(0, dm, ds, dp, dst, ok)
    torch.cuda.synchronize()
    assert int(ok.item()) == 0
    expect_pair_rejected(dst.cpu().numpy(), msg, s2, pk, i, j)


def test_every_row_shifted_with_zero_sum(one_group, rows):
    """Every s_r shifted by a nonzero d_r with sum d_r = 0 (mod l): with equal coefficients the
    whole batch would pass. Every status is 1 and the equation fails."""
    engine = one_group
    n = M.BATCH_MIN
    msg, sig, pk = (a[:n] for a in rows)
    rng = np.random.default_rng(104)
    deltas = [1 + int.from_bytes(rng.bytes(40), "little") % (Z.L - 1) for _ in range(n - 1)]
    deltas.append(-sum(deltas) % Z.L)
    assert all(deltas) and sum(deltas) % Z.L == 0
    s2 = sig.copy()
    for r, d in enumerate(deltas):
        shift_s(s2, r, d)
    st, d = counters_delta(engine, lambda: engine.ed25519_verify(msg, s2, pk))
    assert (st == O.verify_batch(pk, s2, msg)).all() and (st == 1).all()
    assert d == (1, 1, 1, 1)


# ---------------------------------------------------------------- chosen s under small-order keys
def chosen_scalars():
    out = [0, 1, 127, 128, 129, 255, 256, Z.L - 1, Z.L - 2, 1 << 252, (1 << 252) - 1]
    for r in range(32):
        out += [b << (8 * r) for b in (0x80, 0x7F, 0xFF)]            # one such byte at each position
        out += [(128 << (8 * r)) - 1]                                 # 2^(8 r) * 128 (above) and - 1
    for b in (0x80, 0x7F, 0xFF, 0x88):                                # every byte, the top one keeps s < l
        out.append(int.from_bytes(bytes([b] * 31 + [0x0F]), "little"))
    out.append(int.from_bytes(bytes([0x7F, 0x80] * 15 + [0x7F, 0x0F]), "little"))  # alternating
    out.append(int.from_bytes(bytes([0x80, 0x7F] * 15 + [0x80, 0x0F]), "little"))
    rng = np.random.default_rng(105)
    out += [int.from_bytes(rng.bytes(40), "little") % Z.L for _ in range(30)]
    return [s for s in dict.fromkeys(out) if 0 <= s < Z.L]


def flip_one_bit(s, k):
    """s with one bit flipped, still below l (a set bit cleared always is)."""
    for b in range(252):
        t = s ^ (1 << ((7 * k + b) % 253))
        if t < Z.L:
            return t
    raise AssertionError(s)


class Chosen:
    def __init__(self):
        self.s = chosen_scalars()
        n = len(self.s)
        assert 150 <= n <= 260
        self.keys = np.frombuffer(b"".join(e for e, _ in Z.small_order_encodings()), np.uint8).reshape(-1, 32).copy()
        assert any(not c for _, c in Z.small_order_encodings())  # canonical and not
        self.ki = (np.arange(n) % len(self.keys)).astype(np.uint32)
        self.pk = self.keys[self.ki]
        self.msg = np.random.default_rng(106).integers(0, 256, size=(n, 32), dtype=np.uint8)
        r_enc = [Z.compress(Z.scalarmult(Z.B_POINT, s)) for s in self.s]
        self.s_bad = [flip_one_bit(s, k) for k, s in enumerate(self.s)]
        self.sig = self._sigs(r_enc, self.s)
        self.sig_bad = self._sigs(r_enc, self.s_bad)
        # the oracle agrees: accepted as built, rejected with the flipped bit
        assert (O.verify_batch(self.pk, self.sig, self.msg) == 0).all()
        assert (O.verify_batch(self.pk, self.sig_bad, self.msg) == 1).all()

    @staticmethod
    def _sigs(r_enc, scalars):
        return np.frombuffer(b"".join(r + s.to_bytes(32, "little") for r, s in zip(r_enc, scalars)),
                             np.uint8).reshape(-1, 64).copy()


@pytest.fixture(scope="module")
def chosen():
    return Chosen()


def test_chosen_s_on_the_ladder(chosen):
    """k_verify (the effective scalar there is d s mod l: a control)."""
    with M.Engine(devices=(0,), comb=False) as eng:
        assert (eng.ed25519_verify(chosen.msg, chosen.sig, chosen.pk) == 0).all()
        assert (eng.ed25519_verify(chosen.msg, chosen.sig_bad, chosen.pk) == 1).all()


@pytest.mark.parametrize("quad", [0, 1])
def test_chosen_s_on_the_comb_kernels(engine, opts, chosen, quad):
    """k_verify_comb (MV_COMB_QUAD=0) and k_verify_comb16 (1): s recoded into the comb B-table's
    signed digits, row by row."""
    opts("MV_COMB_QUAD", quad)
    engine.set_committee(chosen.keys, np.ones(len(chosen.keys), np.uint64))
    st = engine.ed25519_verify(chosen.msg, chosen.sig, key_idx=chosen.ki)
    assert (st == 0).all(), [hex(chosen.s[i]) for i in np.nonzero(st)[0][:4]]
    st = engine.ed25519_verify(chosen.msg, chosen.sig_bad, key_idx=chosen.ki)
    assert (st == 1).all(), [hex(chosen.s_bad[i]) for i in np.nonzero(st != 1)[0][:4]]


def test_chosen_s_on_the_online_service(engine, chosen):
    """The rows wrapped into blocks (the message is then the block's digest: any message verifies
    under a small-order key), 64 blocks per call on the resident online service."""
    zero_pk = np.frombuffer(O.public_key(B.ZERO_SEED), np.uint8)
    pks = np.concatenate([np.tile(zero_pk, (4, 1)), chosen.keys])
    stakes = np.array([100] * 4 + [1] * len(chosen.keys), np.uint64)
    incs = [b.reference() for b in B.gen_config1(O.sign, rounds=1)]
    bins, want = [], []
    for bad, sigs in ((False, chosen.sig), (True, chosen.sig_bad)):
        for k in range(len(chosen.s)):
            b = B.StatementBlock(4 + int(chosen.ki[k]), 2, incs, [("share", b"chosen s")], 3 * 10**8 + k, False, 0)
            b.signature = sigs[k].tobytes()
            b.digest = b.compute_digest()
            bins.append(b.bincode())
            want.append(M.BLOCK_SIG_INVALID if bad else M.BLOCK_OK)
    for i in (0, len(chosen.s) - 1, len(chosen.s), len(bins) - 1):
        assert O.block_verify(bins[i], pks, stakes, 0)[0] == want[i]
    engine.set_committee(pks, stakes, 0)
    o0 = engine.online_stats()[0]
    calls = 0
    for lo in range(0, len(bins), 64):
        st, _, _ = engine.verify_blocks(bins[lo:lo + 64])
        assert list(st) == want[lo:lo + 64], (lo, [k for k in range(len(st)) if st[k] != want[lo + k]][:4])
        calls += 1
    assert engine.online_stats()[0] - o0 == calls  # every call took the resident service


@pytest.mark.parametrize("committee", [False, True])
def test_chosen_s_on_the_batch_path(one_group, chosen, committee):
    """The forged rows padded with signed rows past BATCH_MIN, as pk rows and as key_idx rows: sum
    z s and -[sum z s]B take every chosen s. All accepted by the equation alone (no fallback); with
    one bit of each s flipped the equation fails and exactly those rows are rejected."""
    engine = one_group
    m = len(chosen.s)
    rng = np.random.default_rng(107)
    pad_msg = rng.integers(0, 256, size=(M.BATCH_MIN, 32), dtype=np.uint8)
    seed = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
    pad_pk, pad_sig = O.sign_batch(np.tile(seed, (M.BATCH_MIN, 1)), pad_msg)
    msg = np.concatenate([chosen.msg, pad_msg])
    pk = np.concatenate([chosen.pk, pad_pk])
    want_bad = np.concatenate([np.ones(m, np.uint8), np.zeros(M.BATCH_MIN, np.uint8)])
    if committee:
        keys = np.concatenate([chosen.keys, pad_pk[:1]])
        engine.set_committee(keys, np.ones(len(keys), np.uint64))
        ki = np.concatenate([chosen.ki, np.full(M.BATCH_MIN, len(keys) - 1, np.uint32)])
        run = lambda sig: engine.ed25519_verify(msg, sig, key_idx=ki)
    else:
        run = lambda sig: engine.ed25519_verify(msg, sig, pk)
    st, d = counters_delta(engine, lambda: run(np.concatenate([chosen.sig, pad_sig])))
    assert (st == 0).all(), [hex(chosen.s[i]) for i in np.nonzero(st[:m])[0][:4]]
    assert d == (1, 0, 1, 0)  # nb == 1, nf == 0
    st, d = counters_delta(engine, lambda: run(np.concatenate([chosen.sig_bad, pad_sig])))
    assert (st == want_bad).all(), np.nonzero(st != want_bad)[0][:8]
    assert d == (1, 1, 1, 1)  # the equation failed
