"""GPU: what the batch path's preparation kernel writes (k_bv_prep, batch.hip), bit-exact against
the plain model of tests/batch_model.py.

The verdict tests (test_gpu_batch.py) cannot see the coefficients z_i of the combined equation: a
valid batch passes it for any z_i, and a batch with one bad signature fails it for any nonzero
ones. The soundness of the batch path rests on the z_i being independent, nonzero 127-bit values,
so the test entry mv_selftest_batch_prep runs the preparation alone -- through the helper the
production path launches it with (launch_prep_stage) -- with a given key, and these tests compare
every output with the model: status, z_i, z_i k_i mod l, the zeroed rows of rejected lanes, the
per-group column sums of z_i s_i, and the affine rows of R and A (as values mod p: the rows are
lazily reduced limbs).
"""
import hashlib

import numpy as np
import pytest

import batch_model as BM
import fe_limbs as FL
import mysticeti_amd as M
import oracle as O
import zip215 as Z

pytestmark = pytest.mark.gpu

N_MIX = 4096 + 17
SIZES = [1, 255, 256, 257, 1023, 1024, 1025, N_MIX]
GROUPS = [1, 3, 8]
LAUNCH_SIGS = [0, 256, 1024]
SECRET = hashlib.sha256(b"prep test secret").digest()
CALL = 0x0123456789ABCDEF  # both counter words in use
L_BYTES = np.frombuffer(Z.L.to_bytes(32, "little"), np.uint8)


def _hex(h, w):
    return np.frombuffer(bytes.fromhex(h), dtype=np.uint8).reshape(w)


def signed_rows(n, seed):
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pk, sig = O.sign_batch(rng.integers(0, 256, size=(n, 32), dtype=np.uint8), msg)
    return msg, sig, pk


def words(v, n):
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(n)]


def expected_scal(model, n):
    return np.array([words(l.z, 4) + words(l.zk, 8) for l in model.lanes[:n]], dtype=np.uint32).reshape(n, 12)


def row_values(row):
    return tuple(FL.value(v) % Z.P for v in FL.quads_to_precomp(row))


class Mix:
    """One batch of 4096 + 17 rows holding every kind of input, its model, and the model's arrays.
    Any prefix of it is a batch of its own with the same model rows (z_i depends on i alone)."""

    def __init__(self, golden):
        msg, sig, pk = (a.copy() for a in signed_rows(N_MIX, 1))
        corpus = golden("zip215_corpus.json")
        # (msg, sig, pk) rows: the corpus' accepts and rejects with 32-byte messages ...
        special = [(_hex(c["msg"], 32), _hex(c["sig"], 64), _hex(c["pk"], 32)) for c in corpus if len(c["msg"]) == 64]
        prerej = []
        bad_r = next(c for c in corpus if c["status"] == 1 and c["note"].startswith("R undecodable"))
        bad_a = next(c for c in corpus if c["status"] == 2)
        for k, kind in enumerate(["s=l", "s bit 255", "R", "A"] * 2):  # explicit pre-rejects
            m, s, a = msg[40 + k].copy(), sig[40 + k].copy(), pk[40 + k].copy()
            if kind == "s=l":
                s[32:] = L_BYTES
            elif kind == "s bit 255":
                s[63] |= 0x80
            elif kind == "R":
                s[:32] = _hex(bad_r["sig"], 64)[:32]
            else:
                a[:] = _hex(bad_a["pk"], 32)
            prerej.append((m, s, a))
        # ... and its small-order pairs (canonical and y >= p encodings, s = 0), whose verdict does
        # not depend on the message
        special += [(np.zeros(32, np.uint8), _hex(c["sig"], 64), _hex(c["pk"], 32)) for c in corpus
                    if len(c["msg"]) != 64]
        special = prerej + special  # (first: they land in the last workgroup too)
        # the last row of every size stays a signed one (a dead lane re-reads it: if dead lanes
        # were summed, a valid row would show), the rest is spread over every workgroup, the ragged
        # last one included
        keep = {n - 1 for n in SIZES}
        spots = [4097, 4098, 4099, 4101, 4103, 4104, 4107, 4111] + [1 + 13 * k for k in range(N_MIX // 13)]
        spots = [p for p in dict.fromkeys(spots) if p not in keep and p < N_MIX]
        assert len(spots) >= len(special)
        for p, (m, s, a) in zip(spots, special):
            msg[p], sig[p], pk[p] = m, s, a
        self.msg, self.sig, self.pk = msg, sig, pk
        self.model = BM.prep(msg, sig, pk, SECRET, CALL)
        self.status = np.array([l.status for l in self.model.lanes], np.uint8)
        self.scal = expected_scal(self.model, N_MIX)
        zs = [l.z * l.s for l in self.model.lanes]
        self.cum = [0]
        for v in zs:
            self.cum.append(self.cum[-1] + v)
        assert {0, 1, 2} == set(self.status.tolist()) and (self.status[4096:] != 0).sum() >= 4
        assert all(self.status[n - 1] == 0 for n in SIZES)

    def sums(self, n, want_groups):
        g, gs = BM.group_geometry(n, want_groups)
        return g, gs, [self.cum[min(n, (k + 1) * gs)] - self.cum[min(n, k * gs)] for k in range(g)]


@pytest.fixture(scope="module")
def mix(golden):
    return Mix(golden)


def check_against_model(out, mx, n, want_groups):
    g, gs, sums = mx.sums(n, want_groups)
    assert (out.groups, out.group_sigs) == (g, gs)
    assert (out.status == mx.status[:n]).all(), np.nonzero(out.status != mx.status[:n])[0][:8]
    assert (out.scal == mx.scal[:n]).all(), np.nonzero((out.scal != mx.scal[:n]).any(axis=1))[0][:8]
    assert not out.scal[mx.status[:n] != 0].any()  # rejected lanes: all-zero rows
    assert [out.group_sum(k) for k in range(g)] == sums
    assert not out.bsum[g:].any()


@pytest.mark.parametrize("n", SIZES)
def test_prep_outputs_match_the_model(engine, mix, n):
    """Every size at which the launch geometry changes (one lane, a workgroup less / exactly /
    plus one, a chunk less / exactly / plus one, four chunks and a ragged workgroup), in 1, 3 and 8
    groups (clamped to the chunk count) and in one launch, 256- and 1024-signature launches:
    status, scalars and group sums equal the model, the three launch forms write identical words,
    and the affine rows of R and A equal the decoded points mod p."""
    msg, sig, pk = mix.msg[:n], mix.sig[:n], mix.pk[:n]
    first = None
    for groups in GROUPS:
        for ls in LAUNCH_SIGS:
            out = engine.batch_prep(msg, sig, pk, groups=groups, secret=SECRET, call=CALL, launch_sigs=ls)
            check_against_model(out, mix, n, groups)
            assert out.a_rows
            if first is None:
                first = out
            else:  # the points do not depend on the geometry: the same words
                assert (out.pts == first.pts).all() and (out.scal == first.scal).all()
    assert (first.pts[:, 27:] == 0).all()
    for i in range(n):
        ln = mix.model.lanes[i]
        if ln.status == 0:
            assert row_values(first.pts[i]) == BM.affine_rows(ln.R), i
            assert row_values(first.pts[n + i]) == BM.affine_rows(ln.A), i


def test_hook_leaves_the_engine_state_alone(engine, mix):
    """The test entry does not count as a batch, and does not use the context's call counter: the
    same key gives the same coefficients before and after production calls."""
    c0, r0 = engine.batch_counters(), engine.batch_routes()
    a = engine.batch_prep(mix.msg[:300], mix.sig[:300], mix.pk[:300], secret=SECRET, call=5)
    assert engine.batch_counters() == c0 and engine.batch_routes() == r0
    msg, sig, pk = signed_rows(M.BATCH_MIN, 2)
    assert (engine.ed25519_verify(msg, sig, pk) == 0).all()
    b = engine.batch_prep(mix.msg[:300], mix.sig[:300], mix.pk[:300], secret=SECRET, call=5)
    assert (a.scal == b.scal).all() and (a.pts == b.pts).all() and (a.bsum == b.bsum).all()


def test_coefficients_are_distinct_nonzero_and_keyed(engine):
    """Over 4096 signed rows with one key: every z_i is nonzero, below 2^127 and distinct, and each
    of the 127 bit positions is set in 40-60 % of them (the true spread is sigma = 0.78 %: a
    condition that keeps a stuck or copied bit from hiding, not a measurement). The next counter
    value, and one flipped bit of the secret, change every z_i; the same key repeats them."""
    n = 4096
    msg, sig, pk = signed_rows(n, 3)
    run = lambda secret, call: engine.batch_prep(msg, sig, pk, secret=secret, call=call)
    base = run(SECRET, 77)
    assert (base.status == 0).all()
    z = [base.z(i) for i in range(n)]
    assert z == [BM.coefficient(SECRET, 77, i) for i in range(n)]
    assert all(0 < v < 1 << 127 for v in z) and len(set(z)) == n
    assert (base.scal[:, 3] >> 31 == 0).all()
    bits = np.unpackbits(np.ascontiguousarray(base.scal[:, :4]).view(np.uint8), axis=1, bitorder="little")
    freq = bits.mean(axis=0)
    assert freq.shape == (128,) and freq[127] == 0
    assert (freq[:127] > 0.40).all() and (freq[:127] < 0.60).all(), (freq.min(), freq.max())
    again = run(SECRET, 77)
    assert (again.scal == base.scal).all() and (again.bsum == base.bsum).all()
    flipped = bytearray(SECRET)
    flipped[31] ^= 0x80
    for other in (run(SECRET, 78), run(SECRET, 77 + (1 << 32)), run(bytes(flipped), 77),
                  run(bytes([SECRET[0] ^ 1]) + SECRET[1:], 77)):
        z2 = [other.z(i) for i in range(n)]
        assert all(a != b for a, b in zip(z, z2))
        assert len(set(z2)) == n and not set(z) & set(z2)


def committee_case(n_keys, bad_at, n=1300, seed=9):
    rng = np.random.default_rng(seed + n_keys)
    seeds = rng.integers(0, 256, size=(n_keys, 32), dtype=np.uint8)
    ki = rng.integers(0, n_keys, size=n).astype(np.uint32)
    ki[:min(n, n_keys)] = np.arange(min(n, n_keys))  # every key of a small committee appears
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pk, sig = O.sign_batch(seeds[ki], msg)
    keys = np.zeros((n_keys, 32), np.uint8)
    for a in range(n_keys):
        rows = np.nonzero(ki == a)[0]
        keys[a] = pk[rows[0]] if len(rows) else O.sign_batch(seeds[a:a + 1], msg[:1])[0][0]
    if bad_at is not None:
        y = next(y for y in range(2, 50) if Z.decompress(y.to_bytes(32, "little")) is None)
        keys[bad_at] = np.frombuffer(y.to_bytes(32, "little"), np.uint8)
    sig = sig.copy()
    sig[5, 32:] = L_BYTES  # a pre-rejected row under a good key (unless that key is the bad one)
    return msg, sig, keys, ki


@pytest.mark.parametrize("n_keys,bad_at", [(1, None), (1, 0), (7, 3), (512, 200)])
def test_committee_forms(engine, opts, n_keys, bad_at):
    """Committee rows (key_idx): A comes from the comb tables of mv_set_committee. Aggregated (the
    default up to 512 keys): no A rows are written; with MV_NO_KEY_AGG the A rows equal the key's
    point. Either way z k, the statuses (2 under the key that does not decode) and the group sums
    equal the model's, in both launch forms."""
    msg, sig, keys, ki = committee_case(n_keys, bad_at)
    n = len(ki)
    ok = engine.set_committee(keys, np.ones(n_keys, np.uint64))
    assert [int(x) for x in ok] == [0 if a == bad_at else 1 for a in range(n_keys)]
    model = BM.prep(msg, sig, keys[ki], SECRET, CALL, groups=2)
    status = np.array([l.status for l in model.lanes], np.uint8)
    assert ((status == 2) == (ki == (-1 if bad_at is None else bad_at))).all()
    assert bad_at == 0 or status[5] == 1
    scal = expected_scal(model, n)
    for agg in (True, False):
        if not agg:
            opts("MV_NO_KEY_AGG", 1)
        for ls in (0, 256):
            out = engine.batch_prep(msg, sig, key_idx=ki, groups=2, secret=SECRET, call=CALL, launch_sigs=ls)
            assert (out.groups, out.group_sigs) == (model.groups, model.group_sigs) == (2, 1024)
            assert (out.status == status).all()
            assert (out.scal == scal).all() and not out.scal[status != 0].any()
            assert [out.group_sum(g) for g in range(2)] == model.sums and not out.bsum[2:].any()
            assert out.a_rows == (not agg)
            if agg:
                assert (out.pts[n:] == M.BATCH_PREP_UNWRITTEN).all()
        for i in range(0, n, 1 if n_keys < 512 else 3):
            ln = model.lanes[i]
            if ln.status == 0:
                assert row_values(out.pts[i]) == BM.affine_rows(ln.R), i
            if not agg and ln.A is not None:  # the key's point, whatever R and s are
                assert row_values(out.pts[n + i]) == BM.affine_rows(ln.A), i
