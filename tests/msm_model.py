"""A plain big-integer model of the batch path's stages after the preparation (batch.hip: the
sort, the buckets, the per-key A term, the reduction and k_bv_final), over oracle/zip215.py's
point arithmetic. Nothing here looks at the engine.

The stages compute, per group g of the batch and per 16-bit window w,

    W[g][w] = sum over the group's signatures i of  dR_i[w] R_i + dA_i[w] A_i,

where dR_i and dA_i are the signed radix-2^16 digits of z_i and of z_i k_i mod l, and then decide

    [8]( sum_w 2^(16 w) W[g][w] + asum[g] - [x_g mod l]B ) == O,

with x_g the integer the group's 12 column sums spell and asum[g] the per-key A term (committee
form, in which the A digits make no entries).

The recoding (the comment at bv_digit / bv_for_digits): a scalar's 16-bit words v_w are walked
from the low end with a carry; v_w + carry >= 2^15 gives the digit v_w + carry - 2^16 and carry 1,
so digits lie in [-2^15, 2^15 - 1]. The top window (7 of the 127-bit z, 15 of z k < l < 2^253) takes
its word plus the carry unsigned, at most 2^15.

To give every window an expected value without a bucket method of its own, the tests use points
with known multiples, P = [a]B + [c]T8 (T8 of order 8): a window's sum is then
[sum d a mod l]B + [sum d c mod 8]T8, one scalar multiplication, and any mix-up of rows changes it.
"""
from collections import Counter

import numpy as np

import fe_limbs as FL
import zip215 as Z

GROUP_CHUNK = 1024
MAX_GROUPS = 16
NWR, NW = 8, 16  # windows of z and of z k
HALF = 1 << 15


# ---- the recoding ----
def _recode(v: int, nwin: int):
    d, carry = [], 0
    for w in range(nwin - 1):
        x = ((v >> (16 * w)) & 0xFFFF) + carry
        carry = 1 if x >= HALF else 0
        d.append(x - (carry << 16))
    d.append((v >> (16 * (nwin - 1))) + carry)  # the top window, unsigned
    return d


def digits(z: int, zk: int):
    """(dR[8], dA[16]) of z < 2^127 and zk < 2^253."""
    assert 0 <= z < 1 << 127 and 0 <= zk < 1 << 253
    return _recode(z, NWR), _recode(zk, NW)


def from_digits(d) -> int:
    return sum(x << (16 * w) for w, x in enumerate(d))


def digits_array(scal):
    """The same for scalar rows (n, 12) uint32: int64 arrays (n, 8) and (n, 16)."""
    scal = np.asarray(scal, dtype=np.uint32)

    def rec(words, nwin):
        h = np.empty((len(words), nwin), np.int64)
        h[:, 0::2] = words & 0xFFFF
        h[:, 1::2] = words >> 16
        carry = np.zeros(len(words), np.int64)
        for w in range(nwin - 1):
            x = h[:, w] + carry
            carry = (x >= HALF).astype(np.int64)
            h[:, w] = x - (carry << 16)
        h[:, nwin - 1] += carry
        return h

    return rec(scal[:, :4].astype(np.int64), NWR), rec(scal[:, 4:].astype(np.int64), NW)


def group_geometry(n: int, want: int):
    """(groups, signatures per group): `want` groups, at most 16 and at most one per 1024-signature
    chunk, of equally many whole chunks; groups left empty are dropped."""
    nchunk = -(-n // GROUP_CHUNK)
    g = min(max(want, 1), MAX_GROUPS, nchunk)
    cpg = -(-nchunk // g)
    return -(-nchunk // cpg), cpg * GROUP_CHUNK


def bucket_occupancy(z, zk, group_sigs, skip_a=False):
    """Counter of (group, window, |digit|) over every bucket entry of the scalar lists."""
    occ = Counter()
    for i, (a, b) in enumerate(zip(z, zk)):
        dr, da = digits(a, b)
        for w, d in enumerate(dr):
            if d:
                occ[(i // group_sigs, w, abs(d))] += 1
        if not skip_a:
            for w, d in enumerate(da):
                if d:
                    occ[(i // group_sigs, w, abs(d))] += 1
    return occ


# ---- points ----
def _find_t8():
    for enc, pt in sorted(Z.torsion_points().items()):
        if not Z.is_identity(Z.double(Z.double(pt))):  # order 8
            return pt
    raise AssertionError("no point of order 8")


T8 = _find_t8()
T8_MULT = [Z.IDENTITY]
for _ in range(7):
    T8_MULT.append(Z.add(T8_MULT[-1], T8))
assert Z.is_identity(Z.add(T8_MULT[7], T8)) and not Z.is_identity(T8_MULT[4])


def affine(pt):
    zi = pow(pt[2], Z.P - 2, Z.P)
    x, y = pt[0] * zi % Z.P, pt[1] * zi % Z.P
    return (x, y, 1, x * y % Z.P)


def affine_many(pts):
    """Affine forms with one inversion for all (Z != 0 on the curve)."""
    pre, acc = [], 1
    for p in pts:
        pre.append(acc)
        acc = acc * p[2] % Z.P
    inv = pow(acc, Z.P - 2, Z.P)
    out = [None] * len(pts)
    for i in range(len(pts) - 1, -1, -1):
        zi = inv * pre[i] % Z.P
        inv = inv * pts[i][2] % Z.P
        x, y = pts[i][0] * zi % Z.P, pts[i][1] * zi % Z.P
        out[i] = (x, y, 1, x * y % Z.P)
    return out


_multiples = [Z.IDENTITY]  # [a]B, affine, built by repeated addition
_multiple_rows = []


def base_multiples(count: int):
    """The affine points [0]B .. [count - 1]B (kept between calls)."""
    if len(_multiples) < count:
        ext, last = [], _multiples[-1]
        for _ in range(count - len(_multiples)):
            last = Z.add(last, Z.B_POINT)
            ext.append(last)
        _multiples.extend(affine_many(ext))
    return _multiples


def known_point(a: int, c: int = 0):
    """[a]B + [c]T8, affine."""
    p = base_multiples(a + 1)[a]
    return affine(Z.add(p, T8_MULT[c % 8])) if c % 8 else p


def known_sum(sa: int, sc: int = 0):
    """[sa mod l]B + [sc mod 8]T8: what a sum of known points must equal."""
    return Z.add(Z.scalarmult(Z.B_POINT, sa % Z.L), T8_MULT[sc % 8])


# ---- rows ----
def point_row(pt):
    """The 32 words of a batch point row: tight canonical limbs of (y+x, y-x, 2dxy), 5 zero words."""
    x, y = pt[0], pt[1]
    assert pt[2] == 1
    vals = ((y + x) % Z.P, (y - x) % Z.P, 2 * Z.D * x * y % Z.P)
    return FL.precomp_to_quads(*(FL.tight(v) for v in vals), quads=8)


def base_multiple_rows(count: int):
    """point_row of [0]B .. [count - 1]B as one (count, 32) uint32 array (kept between calls)."""
    pts = base_multiples(count)
    while len(_multiple_rows) < count:
        _multiple_rows.append(point_row(pts[len(_multiple_rows)]))
    return np.array(_multiple_rows[:count], dtype=np.uint32)


def scalar_row(z: int, zk: int):
    """The 12 words of a scalar row: z in 4, z k in 8."""
    assert 0 <= z < 1 << 127 and 0 <= zk < 1 << 253
    return [(z >> (32 * j)) & 0xFFFFFFFF for j in range(4)] + [(zk >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def scalar_rows(z, zk):
    raw = b"".join(a.to_bytes(16, "little") + b.to_bytes(32, "little") for a, b in zip(z, zk))
    assert all(a < 1 << 127 and b < 1 << 253 for a, b in zip(z, zk))
    return np.frombuffer(raw, dtype="<u4").reshape(len(z), 12).astype(np.uint32)


def decode_p3(row):
    """An extended-point row (36 words: X, Y, Z, T in 9 limbs each, lazily reduced) -> values mod p."""
    w = [int(x) for x in row]
    assert len(w) == 36
    return tuple(FL.value(w[9 * k:9 * k + 9]) % Z.P for k in range(4))


def row_equals(row, pt) -> bool:
    """The device row is the point pt: x = X/Z and y = Y/Z equal pt's exactly mod p, and T Z = X Y."""
    X, Y, Zc, T = decode_p3(row)
    if Zc == 0 or (T * Zc - X * Y) % Z.P:
        return False
    zi = pow(Zc, Z.P - 2, Z.P)
    x, y = affine(pt)[:2]
    return X * zi % Z.P == x and Y * zi % Z.P == y


# ---- the sums ----
def window_sums(z, zk, R, A, group_sigs, skip_a=False):
    """W[g][w] over arbitrary points (lists of extended tuples): the definition, digit by digit."""
    n = len(z)
    groups = -(-n // group_sigs)
    nw = NWR if skip_a else NW
    W = [[Z.IDENTITY] * nw for _ in range(groups)]

    def term(pt, d):
        return Z.scalarmult(pt, d) if d >= 0 else Z.neg(Z.scalarmult(pt, -d))

    for i in range(n):
        g = i // group_sigs
        dr, da = digits(z[i], zk[i])
        for w, d in enumerate(dr):
            if d:
                W[g][w] = Z.add(W[g][w], term(R[i], d))
        if not skip_a:
            for w, d in enumerate(da):
                if d:
                    W[g][w] = Z.add(W[g][w], term(A[i], d))
    return W


def window_scalars(scal, a, c, group_sigs, skip_a=False):
    """For rows of known points (a[i], c[i] for R at i and for A at n + i, small integers): the
    pairs (sum d a mod l, sum d c mod 8) per group and window, from the scalar rows."""
    scal = np.asarray(scal, dtype=np.uint32)
    n = len(scal)
    a, c = np.asarray(a, dtype=np.int64), np.asarray(c, dtype=np.int64)
    assert a.shape == c.shape == (2 * n,) and a.max(initial=0) < 1 << 17 and a.min(initial=0) >= 0
    dR, dA = digits_array(scal)
    out = []
    for lo in range(0, n, group_sigs):
        hi = min(n, lo + group_sigs)
        row = []
        for w in range(NWR if skip_a else NW):
            sa = sc = 0
            if w < NWR:
                sa += int((dR[lo:hi, w] * a[lo:hi]).sum())
                sc += int((dR[lo:hi, w] * c[lo:hi]).sum())
            if not skip_a:
                sa += int((dA[lo:hi, w] * a[n + lo:n + hi]).sum())
                sc += int((dA[lo:hi, w] * c[n + lo:n + hi]).sum())
            row.append((sa % Z.L, sc % 8))
        out.append(row)
    return out


def window_sums_known(scal, a, c, group_sigs, skip_a=False):
    """W[g][w] for rows of known points: one scalar multiplication per window."""
    return [[known_sum(sa, sc) for sa, sc in row] for row in window_scalars(scal, a, c, group_sigs, skip_a)]


def columns_value(cols) -> int:
    """The integer 12 column sums spell (column k weighs 2^(32 k)), carries included."""
    assert len(cols) == 12
    return sum(int(v) << (32 * k) for k, v in enumerate(cols))


def columns_of(x: int, high=(0, 0, 0, 0)):
    """12 columns that spell an integer congruent to x mod l: `high` (64-bit values) in columns
    8..11, the rest of x mod l as 32-bit words in columns 0..7, every second of them folded into
    the column below (so columns 0, 2, 4, 6 carry into their neighbours)."""
    cols = [0] * 8 + [int(h) for h in high]
    assert all(0 <= h < 1 << 64 for h in cols[8:])
    r = (x - columns_value(cols)) % Z.L
    for k in range(8):
        cols[k] = (r >> (32 * k)) & 0xFFFFFFFF
    for k in range(0, 8, 2):
        cols[k] += cols[k + 1] << 32
        cols[k + 1] = 0
    assert (columns_value(cols) - x) % Z.L == 0
    return cols


def combine(W, asum=None):
    """sum_w 2^(16 w) W[w] + asum (Horner from the top window)."""
    acc = Z.IDENTITY
    for w in range(len(W) - 1, -1, -1):
        for _ in range(16):
            acc = Z.double(acc)
        acc = Z.add(acc, W[w])
    return Z.add(acc, asum) if asum is not None else acc


def residual(W, cols, asum=None):
    """sum_w 2^(16 w) W[w] + asum - [x mod l]B."""
    return Z.add(combine(W, asum), Z.neg(Z.scalarmult(Z.B_POINT, columns_value(cols) % Z.L)))


def equation_holds(W, cols, asum=None) -> bool:
    acc = residual(W, cols, asum)
    for _ in range(3):
        acc = Z.double(acc)
    return Z.is_identity(acc)


# ---- chosen scalars: each names the state it puts the stages in (test_msm_model.py checks it) ----
Z_ALL_MIN = from_digits([-HALF] * 7 + [1])            # every window of z at -2^15, the carry runs to window 7
Z_TOP_HALF = from_digits([-HALF] * 7 + [HALF])        # ... and window 7 = 2^15 exactly: 0x7fff plus the carry in
ZK_ALL_MIN = from_digits([-HALF] * 15 + [0x1000])     # every window of z k at -2^15 below a top window of 2^12
ZK_MAX = Z.L - 1                                      # the largest z k: the largest top window, 0x1000


class Rows:
    """A batch for the stages: scalars z[i], zk[i] and known points, R_i = [a[i]]B + [c[i]]T8 and
    A_i = [a[n + i]]B + [c[n + i]]T8 (default: a = 1 .. 2 n, all distinct, c = 0), in `want` groups.
    scal, pts: the rows as k_bv_prep writes them. W: the expected window sums, as points."""

    def __init__(self, z, zk, want=1, a=None, c=None, skip_a=False):
        n = len(z)
        self.n, self.want, self.skip_a = n, want, skip_a
        self.z, self.zk = list(z), list(zk)
        self.a = list(a) if a is not None else list(range(1, 2 * n + 1))
        self.c = list(c) if c is not None else [0] * (2 * n)
        self.groups, self.group_sigs = group_geometry(n, want)
        self.scal = scalar_rows(self.z, self.zk)
        table = base_multiple_rows(max(self.a) + 1)
        self.pts = table[np.asarray(self.a)].copy()
        for i, ci in enumerate(self.c):
            if ci % 8:
                self.pts[i] = point_row(known_point(self.a[i], ci))
        self._w = None

    @property
    def ws(self):
        if self._w is None:
            s = window_scalars(self.scal, self.a, self.c, self.group_sigs, self.skip_a)
            self._w = (s, [[known_sum(sa, sc) for sa, sc in row] for row in s])
        return self._w[0]

    @property
    def W(self):
        self.ws
        return self._w[1]

    def total(self, g: int) -> int:
        """The B multiple of group g's whole sum, sum_w 2^(16 w) (sum d a), mod l."""
        return sum(sa << (16 * w) for w, (sa, _) in enumerate(self.ws[g])) % Z.L

    def balanced(self, extra=None, high=(0, 0, 0, 0)):
        """(16, 12) uint64 columns whose [x]B equals every group's sum of points (plus extra[g] B
        from elsewhere, the per-key term) up to torsion."""
        cols = np.zeros((MAX_GROUPS, 12), dtype=np.uint64)
        for g in range(self.groups):
            cols[g] = columns_of(self.total(g) + (extra[g] if extra else 0), high)
        return cols
