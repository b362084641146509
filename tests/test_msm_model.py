"""CPU: the model of the batch path's stages after the preparation (tests/msm_model.py) is checked
against plain arithmetic before the GPU is judged by it: the recoding sums back to the scalar, the
window sums recombine to the plain multi-scalar sum, the row encoders invert the decoders, each
chosen scalar really makes the state it is named for, and the equation agrees with
batch_model.equation_holds on a preparation of signed inputs."""
import random

import numpy as np

import batch_model as BM
import fe_limbs as FL
import msm_model as MM
import oracle as O
import zip215 as Z

EDGE_Z = [0, 1, MM.HALF - 1, MM.HALF, MM.HALF + 1, 0xFFFF, 0x10000, (1 << 127) - 1, MM.Z_ALL_MIN, MM.Z_TOP_HALF,
          int("7fff" * 8, 16), int("8000" * 7, 16)]
EDGE_ZK = [0, 1, MM.HALF, 0xFFFF, Z.L - 1, Z.L - 2, MM.ZK_ALL_MIN, (1 << 253) - 1, 1 << 252, int("8000" * 15, 16),
           int("0fff" + "ffff" * 15, 16)]


def test_digits_sum_back_and_stay_in_range():
    rng = random.Random(1)
    zs = EDGE_Z + [rng.getrandbits(127) for _ in range(300)]
    zks = EDGE_ZK + [rng.randrange(Z.L) for _ in range(300)]
    for z, zk in zip(zs, zks + zks):
        dr, da = MM.digits(z, zk)
        assert len(dr) == 8 and len(da) == 16
        assert MM.from_digits(dr) == z and MM.from_digits(da) == zk
        assert all(-MM.HALF <= d < MM.HALF for d in dr[:7] + da[:15])
        assert 0 <= dr[7] <= MM.HALF and 0 <= da[15] <= 0x2000
    n = min(len(zs), len(zks))
    dR, dA = MM.digits_array(MM.scalar_rows(zs[:n], zks[:n]))
    for i in range(n):
        dr, da = MM.digits(zs[i], zks[i])
        assert dR[i].tolist() == dr and dA[i].tolist() == da


def test_chosen_scalars_make_the_named_states():
    # every window of z at -2^15 with the carry into window 7; window 7 at 2^15 exactly from 0x7fff
    assert MM.digits(MM.Z_ALL_MIN, 0)[0] == [-MM.HALF] * 7 + [1]
    assert MM.Z_ALL_MIN & 0xFFFF == 0x8000 and MM.Z_ALL_MIN >> 112 == 0
    assert MM.digits(MM.Z_TOP_HALF, 0)[0] == [-MM.HALF] * 7 + [MM.HALF]
    assert MM.Z_TOP_HALF >> 112 == 0x7FFF and MM.Z_TOP_HALF < 1 << 127
    # the same for z k: 15 windows at -2^15 with a carry into window 15; l - 1 has the largest top
    # window a reduced scalar can have (2^15 there would need z k >= 2^255)
    assert MM.digits(0, MM.ZK_ALL_MIN)[1] == [-MM.HALF] * 15 + [0x1000] and MM.ZK_ALL_MIN < Z.L
    assert MM.digits(0, MM.ZK_MAX)[1][15] == 0x1000 == max(MM.digits(0, v)[1][15] for v in EDGE_ZK if v < Z.L)
    # scalars below 2^15 (so below 2^16, and without a carry): windows 1.. have no entry at all
    rng = random.Random(2)
    small = [rng.randrange(1, MM.HALF) for _ in range(64)]
    occ = MM.bucket_occupancy(small, small[::-1], 1024)
    assert {w for _, w, _ in occ} == {0} and sum(occ.values()) == 128
    assert MM.digits(0x8000, 0)[0][:2] == [-MM.HALF, 1]  # (2^15 .. 2^16 - 1 would reach window 1)
    # one z and one z k for all rows: 8 + 16 buckets, each with every row of its group
    z, zk = rng.getrandbits(127), rng.randrange(Z.L)
    occ = MM.bucket_occupancy([z] * 2049, [zk] * 2049, 1024)
    assert len([k for k in occ if k[0] == 0]) == 24 and all(v == (1024 if g < 2 else 1) for (g, _, _), v in occ.items())
    # a group of zero rows has no entries; every other row zero halves them
    occ = MM.bucket_occupancy([0] * 1024 + [z] * 3, [0] * 1024 + [zk] * 3, 1024)
    assert {g for g, _, _ in occ} == {1}
    # T8 has order 8, its fourth multiple order 2
    assert Z.is_identity(Z.scalarmult(MM.T8, 8)) and not Z.is_identity(Z.scalarmult(MM.T8, 4))
    assert Z.is_identity(Z.double(MM.T8_MULT[4])) and Z.point_eq(MM.T8_MULT[3], Z.scalarmult(MM.T8, 3))


def test_known_points_and_row_encoders():
    mult = MM.base_multiples(40)
    for a in (0, 1, 2, 17, 39):
        assert Z.point_eq(mult[a], Z.scalarmult(Z.B_POINT, a)) and mult[a][2] == 1
    assert Z.point_eq(MM.known_point(5, 3), Z.add(Z.scalarmult(Z.B_POINT, 5), Z.scalarmult(MM.T8, 3)))
    assert Z.point_eq(MM.known_sum(Z.L + 7, 11), MM.known_point(7, 3))
    rows = MM.base_multiple_rows(40)
    assert rows.shape == (40, 32) and rows.dtype == np.uint32
    for a in (0, 1, 39):
        row = MM.point_row(mult[a])
        assert rows[a].tolist() == row and len(row) == 32 and not any(row[27:])
        assert all(v < 1 << 29 for v in row)  # tight limbs
        vals = tuple(FL.value(v) for v in FL.quads_to_precomp(row))
        assert vals == BM.affine_rows(mult[a])  # canonical: the values themselves, below p
    assert rows[0].tolist()[:10] == [1] + [0] * 8 + [1]  # the identity: (1, 1, 0)
    z, zk = (1 << 127) - 5, Z.L - 1
    row = MM.scalar_row(z, zk)
    assert MM.scalar_rows([z], [zk])[0].tolist() == row
    assert int.from_bytes(np.array(row[:4], np.uint32).tobytes(), "little") == z
    assert int.from_bytes(np.array(row[4:], np.uint32).tobytes(), "little") == zk
    # an extended row in any limb form decodes to the point; a wrong T or another point does not
    pt = Z.scalarmult(Z.B_POINT, 12345)
    ext = [v * 7 % Z.P for v in pt]  # another Z
    limbs = sum((FL.borrowed(FL.tight(v)) for v in ext), [])
    assert MM.row_equals(limbs, pt) and MM.row_equals(limbs, MM.affine(pt))
    assert not MM.row_equals(limbs, Z.scalarmult(Z.B_POINT, 12346))
    assert not MM.row_equals(limbs, Z.neg(pt))
    bad = list(limbs)
    bad[27] ^= 1
    assert not MM.row_equals(bad, pt)


def test_window_sums_recombine_to_the_plain_sum():
    rng = random.Random(3)
    n = 6
    zs = [rng.getrandbits(127) for _ in range(n - 2)] + [MM.Z_TOP_HALF, 0]
    zks = [rng.randrange(Z.L) for _ in range(n - 2)] + [MM.ZK_MAX, 0]
    rows = MM.Rows(zs, zks, c=[(3 * i + 1) % 8 for i in range(2 * n)])
    R = [MM.known_point(rows.a[i], rows.c[i]) for i in range(n)]
    A = [MM.known_point(rows.a[n + i], rows.c[n + i]) for i in range(n)]
    W = MM.window_sums(zs, zks, R, A, rows.group_sigs)
    assert len(W) == 1 and len(W[0]) == 16
    for w in range(16):  # the one-multiplication form equals the definition
        assert Z.point_eq(W[0][w], rows.W[0][w]), w
    plain = Z.IDENTITY
    for i in range(n):
        plain = Z.add(plain, Z.add(Z.scalarmult(R[i], zs[i]), Z.scalarmult(A[i], zks[i])))
    assert Z.point_eq(MM.combine(W[0]), plain)
    # balanced columns make the equation hold; one more B, or one less, does not; torsion does
    cols = rows.balanced(high=(2**64 - 1, 2**63, 5, 2**64 - 1))[0]
    assert MM.equation_holds(W[0], cols)
    res = MM.residual(W[0], cols)
    assert Z.is_identity(Z.scalarmult(res, 8)) and not Z.is_identity(res)  # (a torsion point is left)
    off = cols.copy()
    off[0] += np.uint64(1)
    assert not MM.equation_holds(W[0], off)
    # the per-key form: no A entries, their term arrives as asum
    WR = MM.window_sums(zs, zks, R, A, rows.group_sigs, skip_a=True)
    assert len(WR[0]) == 8
    asum = Z.IDENTITY
    for i in range(n):
        asum = Z.add(asum, Z.scalarmult(A[i], zks[i]))
    assert Z.point_eq(MM.combine(WR[0], asum), plain)
    assert MM.equation_holds(WR[0], cols, asum) and not MM.equation_holds(WR[0], cols)
    assert MM.window_scalars(rows.scal, rows.a, rows.c, rows.group_sigs, skip_a=True)[0] != rows.ws[0][:8]


def test_columns():
    assert MM.columns_value([2**64 - 1] * 12) == (2**64 - 1) * sum(1 << (32 * k) for k in range(12))
    for x in (0, 1, Z.L - 1, 12345 << 200):
        for high in ((0, 0, 0, 0), (2**64 - 1,) * 4):
            cols = MM.columns_of(x, high)
            assert (MM.columns_value(cols) - x) % Z.L == 0 and all(0 <= c < 1 << 64 for c in cols)


def test_groups_split_the_sums():
    assert [MM.group_geometry(n, w) for n, w in ((1, 3), (1025, 1), (2049, 2), (4096, 16), (16384, 16), (4096, 3))] == \
        [(1, 1024), (1, 2048), (2, 2048), (4, 1024), (16, 1024), (2, 2048)]
    assert all(MM.group_geometry(n, w) == BM.group_geometry(n, w) for n in (1, 1024, 1025, 5000) for w in (0, 1, 2, 7, 40))
    rng = random.Random(4)
    n = 1027
    rows = MM.Rows([rng.getrandbits(127) for _ in range(n)], [rng.randrange(Z.L) for _ in range(n)], want=2)
    assert (rows.groups, rows.group_sigs) == (2, 1024) and len(rows.W) == 2
    tot = sum(rows.z[i] * rows.a[i] + rows.zk[i] * rows.a[n + i] for i in range(1024, n)) % Z.L
    assert rows.total(1) == tot
    assert Z.point_eq(MM.combine(rows.W[1]), Z.scalarmult(Z.B_POINT, tot))


def test_equation_agrees_with_the_preparation_model():
    rng = np.random.default_rng(5)
    n = 5
    msg = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pk, sig = O.sign_batch(rng.integers(0, 256, size=(n, 32), dtype=np.uint8), msg)
    for bad in (None, 3):
        sg = sig.copy()
        if bad is not None:
            sg[bad, 40] ^= 1
        p = BM.prep(msg, sg, pk, bytes(32), 9)
        lanes = p.lanes
        W = MM.window_sums([l.z for l in lanes], [l.zk for l in lanes], [l.R for l in lanes], [l.A for l in lanes],
                           p.group_sigs)
        cols = [(p.sums[0] >> (32 * k)) & 0xFFFFFFFF for k in range(12)]
        cols[11] = p.sums[0] >> (32 * 11)
        assert MM.equation_holds(W[0], cols) == BM.equation_holds(p, 0) == (bad is None)
