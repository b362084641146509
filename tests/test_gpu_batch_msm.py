"""GPU: the batch path's stages after the preparation (batch.hip: k_part_*, k_fine_sort_lds,
k_bv_bucket_*, k_bv_key*, k_bv_reduce*, k_bv_final) against the plain model of tests/msm_model.py.

The verdict tests see these stages through two observations only: a valid batch passes without a
fallback, and a batch with a bad signature comes back exact. A wrong sum shows there as a silent
fallback, and a sum that lost a whole group or window range can pass as the identity. The test
entry mv_selftest_batch_msm runs the stages alone -- through the helper the production path
launches them with (launch_msm_stage) -- on chosen scalars, points with known multiples
([a]B + [c]T8) and chosen column sums, and these tests compare every group's every window sum
with the model exactly (x = X/Z, y = Y/Z mod p, T Z = X Y) and every flag with the model's
equation, so a failure names the stage's output, the group and the window.
"""
import functools
import hashlib
import random

import numpy as np
import pytest

import batch_model as BM
import msm_model as MM
import oracle as O
import zip215 as Z

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 1024, 1025, 2049, 4096]


def rand_scalars(n, seed):
    rng = random.Random(seed)
    return [rng.getrandbits(127) for _ in range(n)], [rng.randrange(Z.L) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def random_rows(n, want):
    return MM.Rows(*rand_scalars(n, 100 + n), want=want)


def check(engine, rows, cols=None, expect=None):
    """Runs the stages on rows with the column sums cols (default: balanced, so every flag must be
    1) and compares geometry, every window sum and every flag with the model."""
    cols = rows.balanced() if cols is None else cols
    out = engine.batch_msm(rows.scal, rows.pts, cols, groups=rows.want)
    assert (out.groups, out.group_sigs) == (rows.groups, rows.group_sigs)
    W = rows.W
    assert out.win.shape == (rows.groups, len(W[0]), 36)
    wrong = [(g, w) for g in range(rows.groups) for w in range(len(W[g])) if not MM.row_equals(out.win[g, w], W[g][w])]
    assert not wrong, f"window sums differ from the model at (group, window) {wrong[:12]}"
    flags = [int(MM.equation_holds(W[g], cols[g])) for g in range(rows.groups)]
    if expect is not None:
        assert flags == expect  # what the case was built to show
    assert out.flags == flags and out.flag_all == int(all(flags))
    return out


@pytest.mark.parametrize("want", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_random_scalars_every_size(engine, n, want):
    """One lane, less than a workgroup, a chunk exactly / plus one, two chunks plus one (a second
    group of one signature), four chunks; balanced column sums: every flag 1."""
    rows = random_rows(n, want)
    check(engine, rows, expect=[1] * rows.groups)


@pytest.mark.parametrize("n,groups", [(4096, 4), (16384, 16)])
def test_sixteen_groups_wanted(engine, n, groups):
    rows = random_rows(n, 16)
    assert rows.groups == groups
    check(engine, rows, expect=[1] * groups)
    if groups == 16:  # one group's column sums off by one B: that flag alone falls (k_bv_final, g >= 8)
        for g in (9, 15):
            cols = rows.balanced()
            cols[g, 0] += np.uint64(1)
            check(engine, rows, cols, expect=[int(k != g) for k in range(16)])


def _edge_rows(name):
    n = 1025
    z, zk = rand_scalars(n, 7)
    a = c = None
    want = 2
    if name == "z_all_windows_min":
        z = [MM.Z_ALL_MIN] * n
    elif name == "z_top_window_half":
        z = [MM.Z_TOP_HALF if i % 3 else z[i] for i in range(n)]
    elif name == "zk_all_windows_min":
        zk = [MM.ZK_ALL_MIN] * n
    elif name == "zk_largest":
        zk = [MM.ZK_MAX if i % 3 else zk[i] for i in range(n)]
    elif name == "small_scalars":
        z, zk = [v % MM.HALF for v in z], [v % MM.HALF for v in zk]
    elif name == "zero_group":
        n, want = 3072, 3
        z, zk = rand_scalars(n, 8)
        z[1024:2048] = zk[1024:2048] = [0] * 1024
    elif name == "every_other_row_zero":
        z, zk = [v * (i & 1) for i, v in enumerate(z)], [v * (i & 1) for i, v in enumerate(zk)]
    elif name == "one_scalar_for_all":
        n, want = 4096, 1
        z, zk = [z[0]] * n, [zk[0]] * n
    elif name == "one_scalar_one_point":
        n = 2049
        z, zk = [z[0]] * n, [zk[0]] * n
        a = [3] * n + [5] * n
    elif name == "torsion_parts":
        n, want = 255, 1
        z, zk = z[:n], zk[:n]
        c = [1 + i % 7 for i in range(n)] + [(3 * i) % 8 for i in range(n)]
    elif name == "identity_a_row":
        n, want = 255, 1
        z, zk = z[:n], zk[:n]
        a = list(range(1, 2 * n + 1))
        a[n + 5] = a[n + 254] = 0
    else:
        raise KeyError(name)
    return MM.Rows(z, zk, want=want, a=a, c=c)


EDGES = ["z_all_windows_min", "z_top_window_half", "zk_all_windows_min", "zk_largest", "small_scalars", "zero_group",
         "every_other_row_zero", "one_scalar_for_all", "one_scalar_one_point", "torsion_parts", "identity_a_row"]


@functools.lru_cache(maxsize=None)
def edge_rows(name):
    return _edge_rows(name)


@pytest.mark.parametrize("name", EDGES)
def test_chosen_scalars(engine, name):
    """One state the code has a rule for per case (test_msm_model.py shows that the scalars make it):
    digits of -2^15 with the carry through every window, the unsigned top windows at their largest,
    empty windows, a group and rows without entries, buckets that span many lanes of the balanced
    bucket kernel, the same point n times in a bucket (P + P), torsion parts, the identity as A."""
    rows = edge_rows(name)
    if name == "one_scalar_for_all":
        occ = MM.bucket_occupancy(rows.z[:2], rows.zk[:2], rows.group_sigs)
        assert len(occ) == 24 and set(occ.values()) == {2}  # 24 buckets hold all 24 n entries
    check(engine, rows, expect=[1] * rows.groups)
    if name == "zero_group":
        assert all(Z.is_identity(p) for p in rows.W[1])
        cols = rows.balanced()
        assert not cols[1].any()
        cols[1, 0] = 1  # no entries and a nonzero sum z s: [1]B is left
        check(engine, rows, cols, expect=[1, 0, 1])
        cols[1] = [int(v) for v in MM.columns_of(0, (7, 0, 0, 2**63))]  # a multiple of l: nothing is left
        check(engine, rows, cols, expect=[1, 1, 1])


FORMS = [("MV_BUCKET_BAL", 1), ("MV_BUCKET_BAL", 8), ("MV_REDUCE_QUAD", 0), ("MV_REDUCE_QUAD", None),
         ("MV_REDUCE_ROWS", 0), ("MV_REDUCE_ROWS", None), ("MV_FINAL_ROWS", 0), ("MV_FINAL_ROWS", 1)]


@pytest.mark.parametrize("knob,value", FORMS, ids=[f"{k}={'default' if v is None else v}" for k, v in FORMS])
def test_every_kernel_form(engine, opts, knob, value):
    """The random case (one group, and two groups with a second of one signature) and the one-scalar
    case under every kernel form the options select: the same window sums and flags."""
    if value is not None:
        opts(knob, value)
    for rows in (random_rows(4096, 1), random_rows(2049, 2), edge_rows("one_scalar_for_all"),
                 edge_rows("one_scalar_one_point")):
        check(engine, rows, expect=[1] * rows.groups)
    rows = random_rows(2049, 2)
    cols = rows.balanced()
    cols[0, 3] ^= np.uint64(1 << 40)
    check(engine, rows, cols, expect=[0, 1])


def test_flags_follow_the_sum(engine):
    """A known non-identity sum must give flag 0, in the group it is in and in no other: one window's
    worth of one row changed (every window of z and of z k in turn, rows at both ends of a group);
    [1]B left over; and flag 1 where only a torsion point is left (T8, the point of order 2)."""
    n = 3072
    base = random_rows(n, 3)
    cols = base.balanced()
    for k, (row, half) in enumerate([(0, 0), (1023, 7), (1024, 3), (2047, 8), (2048, 15), (3071, 23), (1500, 22)]):
        z, zk = list(base.z), list(base.zk)
        if half < 8:
            z[row] ^= 1 << (16 * half + k)
        else:
            zk[row] ^= 1 << (16 * (half - 8) + k)
        g = row // 1024
        check(engine, MM.Rows(z, zk, want=3), cols, expect=[int(x != g) for x in range(3)])
    # [1]B left in group 2
    off = cols.copy()
    off[2] = MM.columns_of(base.total(2) - 1)
    res = MM.residual(base.W[2], off[2])
    assert Z.point_eq(res, Z.B_POINT)
    check(engine, base, off, expect=[1, 1, 0])
    # T8 and the point of order 2 left: the cofactor clears them
    for c_left in (1, 4):
        z, zk = rand_scalars(255, 11)
        z[17] |= 1
        z[17] ^= (z[17] & 7) ^ 1  # z = 1 mod 8 on the only row with a torsion part
        c = [0] * 510
        c[17] = c_left
        rows = MM.Rows(z, zk, c=c)
        res = MM.residual(rows.W[0], rows.balanced()[0])
        assert Z.point_eq(res, MM.T8_MULT[c_left]) and not Z.is_identity(res)
        check(engine, rows, expect=[1])


@pytest.mark.parametrize("col", [2**64 - 1, 2**63])
def test_column_sums_at_their_bounds(engine, col):
    """All 12 column sums at 2^64 - 1 and at 2^63 (k_bv_final's carry chain into x[12], x[13] and
    sc_reduce512): the scalars are chosen so that the points' sum is exactly [x mod l]B, so the flag
    must be 1, and 0 with one less in any single column."""
    cols = np.zeros((16, 12), dtype=np.uint64)
    cols[0] = col
    x = MM.columns_value([col] * 12) % Z.L
    z = 12345
    rows = MM.Rows([z], [(x - z) * pow(2, -1, Z.L) % Z.L])  # R = [1]B, A = [2]B: z + 2 zk = x mod l
    assert rows.total(0) == x
    check(engine, rows, cols, expect=[1])
    for k in (0, 5, 11):
        off = cols.copy()
        off[0, k] -= np.uint64(1)
        check(engine, rows, off, expect=[0])


def committee(n_keys):
    """Keys A_b = [5000 + b]B: (encodings, multiples)."""
    mult = MM.base_multiples(5000 + n_keys)
    return np.array([np.frombuffer(Z.compress(mult[5000 + b]), np.uint8) for b in range(n_keys)]), \
        [5000 + b for b in range(n_keys)]


@pytest.mark.parametrize("n_keys", [3, 512])
def test_per_key_form(engine, n_keys):
    """The committee form: no A entries, A's term summed per key (k_bv_keyacc, k_bv_keycol,
    k_bv_keysum). n = 4096 in 2 groups of 2 chunks; one key has z k = l - 1 on every row, a whole chunk of them
    (the largest column sums); one key has no rows; keys are spread unevenly over the groups. asum
    must equal sum_b [sum z k mod l] A_b per group, the R window sums the model's, the flags 1 with
    balanced columns, and 0 in the one group whose key sum was changed."""
    n, want = 4096, 2
    keys, kmult = committee(n_keys)
    ok = engine.set_committee(keys, np.ones(n_keys, np.uint64))
    assert all(int(x) for x in ok)
    rng = np.random.default_rng(n_keys)
    hot, dead = 1, 2 if n_keys == 3 else 300
    ki = rng.integers(0, n_keys, size=n).astype(np.uint32)
    ki[:1024] = ki[:1024] % min(n_keys, 5)          # the first chunk uses few keys,
    ki[1024:2048] = hot                               # the second one key alone,
    ki[3072:] = np.minimum(ki[3072:], n_keys - 1 - (np.arange(1024) % 2))  # the last leans on the last keys
    ki[ki == dead] = 0
    assert not (ki == dead).any() and (ki == hot).sum() >= 1024
    z, zk = rand_scalars(n, 12)
    zk = [MM.ZK_MAX if ki[i] == hot else v for i, v in enumerate(zk)]
    rows = MM.Rows(z, zk, want=want, skip_a=True)
    G, gs = rows.groups, rows.group_sigs
    assert (G, gs) == (2, 2048)  # two chunks per group: k_bv_keycol sums over chunks
    extra, asum = [], []
    for g in range(G):
        per_key = [0] * n_keys
        for i in range(gs * g, gs * (g + 1)):
            per_key[ki[i]] += zk[i]
        if g == 0:
            assert per_key[hot] >= 1024 * MM.ZK_MAX
        extra.append(sum((v % Z.L) * kmult[b] for b, v in enumerate(per_key)) % Z.L)
        asum.append(Z.scalarmult(Z.B_POINT, extra[-1]))
    cols = rows.balanced(extra=extra, high=(2**64 - 1, 1, 0, 2**62))
    for changed in (None, 1):
        sk = rows.scal.copy()
        exp = [1] * G
        asum_x = list(asum)
        if changed is not None:  # one word of one z k in the last chunk: the R sums stay, the key sum moves
            i = 3072 + 77
            sk[i, 6] ^= 1
            d = (int.from_bytes(sk[i, 4:].tobytes(), "little") - zk[i]) % Z.L
            asum_x[1] = Z.add(asum[1], Z.scalarmult(Z.B_POINT, d * kmult[ki[i]] % Z.L))
            exp[1] = 0
        out = engine.batch_msm(sk, rows.pts[:n], cols, groups=want, key_idx=ki, n_keys=n_keys)
        assert (out.groups, out.group_sigs) == (G, gs) and out.win.shape == (G, 8, 36)
        wrong = [(g, w) for g in range(G) for w in range(8) if not MM.row_equals(out.win[g, w], rows.W[g][w])]
        assert not wrong, wrong
        bad = [g for g in range(G) if not MM.row_equals(out.asum[g], asum_x[g])]
        assert not bad, f"asum differs from the model in groups {bad}"
        assert [int(MM.equation_holds(rows.W[g], cols[g], asum_x[g])) for g in range(G)] == exp
        assert out.flags == exp and out.flag_all == int(all(exp))


def test_joined_to_the_real_preparation(engine):
    """Engine.batch_prep's own scal, pts and bsum of a signed batch with one corrupted signature, fed
    in unchanged: a group of 1024 valid signatures must pass and the group with the bad one fail, as
    batch_model.equation_holds says."""
    n = 1025
    rng = np.random.default_rng(21)
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pk, sig = O.sign_batch(rng.integers(0, 256, size=(n, 32), dtype=np.uint8), msg)
    sig = sig.copy()
    sig[1024, 40] ^= 0x10  # s stays below l: the preparation accepts it, only the equation sees it
    secret = hashlib.sha256(b"msm joined").digest()
    prep = engine.batch_prep(msg, sig, pk, groups=2, secret=secret, call=3)
    assert (prep.status == 0).all() and (prep.groups, prep.group_sigs) == (2, 1024)
    model = BM.prep(msg, sig, pk, secret, 3, groups=2)
    exp = [int(BM.equation_holds(model, g)) for g in range(2)]
    assert exp == [1, 0]
    out = engine.batch_msm(prep.scal, prep.pts, prep.bsum, groups=2)
    assert out.flags == exp and out.flag_all == 0
    # and the window sums are the model's over the real points
    lanes = model.lanes[1024:]
    W = MM.window_sums([l.z for l in lanes], [l.zk for l in lanes], [l.R for l in lanes], [l.A for l in lanes], 1024)
    assert all(MM.row_equals(out.win[1, w], W[0][w]) for w in range(16))


def test_entry_leaves_the_engine_state_alone_and_checks_its_input(engine):
    import mysticeti_amd as M

    rows = random_rows(255, 1)
    c0, r0 = engine.batch_counters(), engine.batch_routes()
    check(engine, rows)
    assert engine.batch_counters() == c0 and engine.batch_routes() == r0
    bad = rows.scal.copy()
    bad[3, 3] |= 1 << 31  # z >= 2^127: its top digit would leave the key space
    with pytest.raises(M.MvError):
        engine.batch_msm(bad, rows.pts, rows.balanced())
    bad = rows.scal.copy()
    bad[3, 11] |= 1 << 29
    with pytest.raises(M.MvError):
        engine.batch_msm(bad, rows.pts, rows.balanced())
