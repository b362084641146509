"""ORACLE / TEST INFRASTRUCTURE ONLY — never imported by the product path.

Word-exact model of the lazy limb arithmetic of mysticeti_amd/csrc/fe25519.h, fe_q4.h,
fe_r16.h and pt_r16.h: 9 limbs of 29 bits held in 32-bit words, 64-bit column sums. Every
function does what the HIP code does, wrap-around included, and reports where a 32- or 64-bit
quantity would wrap: with strict=True (the default) that raises ContractError, so a test knows
a chosen input is inside the code's contract before it judges the GPU's result; with
strict=False the value wraps as the hardware would.

The value of a limb vector is sum(limb[i] << 29 i).
"""
from __future__ import annotations

P = 2**255 - 19
M29 = (1 << 29) - 1
U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
R261 = 1216  # 2^261 mod p
N_BOUND = 2**29 + 2**23  # "N": every limb below this
A_BOUND = 2**30 + 2**24  # "A": every limb below this
NORM_IN_MAX = 2**32 - 8  # fe_normalize: the largest limb for which no carry wraps
SUB_BIAS = [0x7FFFED00] + [0x7FFFFFFC] * 8  # 16 p in limbs


class ContractError(AssertionError):
    pass


def value(limbs) -> int:
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def tight(v: int):
    """The limb vector of v < 2^261 with every limb < 2^29."""
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & M29 for i in range(9)]


def greedy(v: int, bound: int):
    """A limb vector of v with every limb < bound, high limbs as large as possible; None if v
    does not fit."""
    out = [0] * 9
    for i in range(8, 0, -1):
        out[i] = min(bound - 1, v >> (29 * i))
        v -= out[i] << (29 * i)
    if v >= bound:
        return None
    out[0] = v
    return out


def borrowed(limbs):
    """The same value with 2^29 moved down from every limb that can spare 1: limbs 0..7 in
    [2^29, 2^30) wherever the limb above is not zero."""
    out = list(limbs)
    for i in range(8):
        if out[i + 1] >= 1:
            out[i + 1] -= 1
            out[i] += 1 << 29
    return out


def _u32(x, strict, what):
    if x > U32 or x < 0:
        if strict:
            raise ContractError(f"{what}: 32-bit wrap ({x:#x})")
        x &= U32
    return x


def _u64(x, strict, what):
    if x > U64:
        if strict:
            raise ContractError(f"{what}: 64-bit wrap ({x:#x})")
        x &= U64
    return x


# ---- fe25519.h ----
def normalize(a, strict=True):
    r = list(a)
    for i in range(8):
        c = r[i] >> 29
        r[i] &= M29
        r[i + 1] = _u32(r[i + 1] + c, strict, f"fe_normalize limb {i + 1}")
    c = r[8] >> 29
    r[8] &= M29
    r[0] = _u32(r[0] + c * R261, strict, "fe_normalize limb 0")
    return r


def add(a, b, strict=True):
    return [_u32(x + y, strict, "fe_add") for x, y in zip(a, b)]


def addn(a, b, strict=True):
    return normalize(add(a, b, strict), strict)


def _sub_raw(a, b, strict, what):
    r = []
    for x, y, c in zip(a, b, SUB_BIAS):
        if y > c and strict:
            raise ContractError(f"{what}: subtrahend limb above the bias")
        r.append(_u32(x + ((c - y) & U32), strict, what))
    return r


def sub(a, b, strict=True):
    return normalize(_sub_raw(a, b, strict, "fe_sub"), strict)


def neg(a, strict=True):
    return sub([0] * 9, a, strict)


def _reduce_scan(cols, strict):
    lo = [_u64(c, strict, "column") for c in cols[:9]]
    for k in range(9, 17):
        c = _u64(cols[k], strict, "column")
        lo[k - 9] = _u64(lo[k - 9] + (c & U32) * R261, strict, "fold")
        lo[k - 8] = _u64(lo[k - 8] + (c >> 32) * (8 * R261), strict, "fold")
    r = [0] * 9
    for k in range(8):
        r[k] = lo[k] & M29
        lo[k + 1] = _u64(lo[k + 1] + (lo[k] >> 29), strict, "carry")
    r[8] = lo[8] & M29
    t0 = _u64(r[0] + (lo[8] >> 29) * R261, strict, "top fold")
    r[0] = t0 & M29
    r[1] = _u32(r[1] + _u32(t0 >> 29, strict, "top fold carry"), strict, "top fold carry")
    return r


def _columns(a, b):
    cols = [0] * 17
    for i in range(9):
        for j in range(9):
            cols[i + j] += a[i] * b[j]
    return cols


def mul(a, b, strict=True):
    return _reduce_scan(_columns(a, b), strict)


def sq(a, strict=True):
    a2 = [_u32(x << 1, strict, "fe_sq doubled limb") for x in a]
    cols = [0] * 17
    for k in range(17):
        c = 0 if k & 1 else a[k >> 1] * a[k >> 1]
        i = max(k - 8, 0)
        while i < k - i:
            c += a2[i] * a[k - i]
            i += 1
        cols[k] = c
    return _reduce_scan(cols, strict)


def sqn(a, n, strict=True):
    for _ in range(n):
        a = sq(a, strict)
    return a


def mul_small(a, c, strict=True):
    t = [_u64(x * c, strict, "fe_mul_small") for x in a]
    r = [0] * 9
    for k in range(8):
        r[k] = t[k] & M29
        t[k + 1] = _u64(t[k + 1] + (t[k] >> 29), strict, "fe_mul_small carry")
    r[8] = t[8] & M29
    t0 = r[0] + (t[8] >> 29) * R261
    r[0] = t0 & M29
    r[1] = _u32(r[1] + (t0 >> 29), strict, "fe_mul_small top")
    return r


def canon(a, strict=True, folds=2):
    t = normalize(a, strict)
    for _ in range(folds):
        q = t[8] >> 23
        t[8] &= (1 << 23) - 1
        t[0] = _u32(t[0] + q * 19, strict, "fe_canon fold")
        for i in range(8):
            c = t[i] >> 29
            t[i] &= M29
            t[i + 1] = _u32(t[i + 1] + c, strict, "fe_canon carry")
    u = [0] * 9
    c = 19
    for i in range(9):
        s = t[i] + c
        c = s >> 29
        u[i] = s & M29
    ge = (u[8] >> 23) != 0
    u[8] &= (1 << 23) - 1
    return u if ge else t


def is_zero(a, strict=True):
    return not any(canon(a, strict))


def is_negative(a, strict=True):
    return bool(canon(a, strict)[0] & 1)


def eq(a, b, strict=True):
    return is_zero(sub(a, b, strict), strict)


def to_words(a, strict=True):
    v = value(canon(a, strict))
    return [(v >> (32 * j)) & U32 for j in range(8)]


# ---- fe_q4.h: four lanes per element, lane c holds limbs c, 4 + c and (lane 0) 8 ----
def feq_mul(a, b, strict=True):
    full = _columns(a, b) + [0] * 3  # columns 0..19
    col = [[_u64(full[4 * r + c], strict, "column") for r in range(5)] for c in range(4)]
    lo = [[0, 0, 0] for _ in range(4)]
    s = [[0, 0] for _ in range(4)]
    for c in range(4):
        h2 = 0 if c == 0 else col[c][2]
        lo[c][0] = _u64(col[c][0] + (h2 >> 32) * (8 * R261), strict, "fold")
        lo[c][1] = _u64(col[c][1] + (col[c][3] >> 32) * (8 * R261), strict, "fold")
        lo[c][2] = _u64((col[c][2] if c == 0 else 0) + (col[c][4] >> 32) * (8 * R261), strict, "fold")
        f2, f3, f4 = (h2 & U32) * R261, (col[c][3] & U32) * R261, (col[c][4] & U32) * R261
        s[c] = [f3, f4] if c == 0 else [f2, f3]
    for c in range(4):
        lo[c][0] = _u64(lo[c][0] + s[(c + 1) & 3][0], strict, "fold")
        lo[c][1] = _u64(lo[c][1] + s[(c + 1) & 3][1], strict, "fold")
    # carry round 1 (64-bit)
    k = [[x >> 29 for x in lo[c]] for c in range(4)]
    for c in range(4):
        g0, g1 = k[(c + 3) & 3][0], k[(c + 3) & 3][1]
        w = _u64(k[c][2] * R261, strict, "wrap")
        lo[c][0] = _u64((lo[c][0] & M29) + (w if c == 0 else g0), strict, "carry 1")
        lo[c][1] = _u64((lo[c][1] & M29) + (g0 if c == 0 else g1), strict, "carry 1")
        lo[c][2] = _u64((lo[c][2] & M29) + (g1 if c == 0 else 0), strict, "carry 1")
    # carry round 2 (32-bit carries)
    k = [[_u32(x >> 29, strict, "carry 2 width") for x in lo[c]] for c in range(4)]
    out = [0] * 9
    for c in range(4):
        g0, g1 = k[(c + 3) & 3][0], k[(c + 3) & 3][1]
        r0 = (lo[c][0] & M29) + (_u32(k[c][2] * R261, strict, "carry 2 wrap") if c == 0 else g0)
        r1 = (lo[c][1] & M29) + (g0 if c == 0 else g1)
        out[c] = _u32(r0, strict, "carry 2")
        out[4 + c] = _u32(r1, strict, "carry 2")
        if c == 0:
            out[8] = _u32((lo[c][2] & M29) + g1, strict, "carry 2")
    return out


def feq_sqn(a, n, strict=True):
    for _ in range(n):
        a = feq_mul(a, a, strict)
    return a


# ---- fe_r16.h: lane t of a 16-lane row holds limb t ----
def fer_mul(a, b, strict=True):
    full = [_u64(c, strict, "column") for c in _columns(a, b)]
    col, c16 = full[:16], full[16]
    lo = [c & U32 for c in col]
    hi = [c >> 32 for c in col]
    v = [0] * 9
    for t in range(9):
        x = col[t] + (lo[t + 9] if t + 9 < 16 else 0) * R261
        x += (hi[t + 8] if t + 8 < 16 else 0) * (8 * R261 if 1 <= t <= 7 else 0)
        x += (c16 & U32) * (R261 if t == 7 else 0)
        x += (c16 >> 32) * (8 * R261 if t == 8 else 0)
        v[t] = _u64(x, strict, "fold")
    vl = [x & U32 for x in v]
    vh = [x >> 32 for x in v]
    w = [0] * 9
    for t in range(9):
        x = vl[t] + ((vh[t - 1] << 3) if t >= 1 else 0)
        x += vh[8] * (8 * R261) if t == 0 else 0
        w[t] = _u64(x, strict, "carry 1")
    kk = [_u32(x >> 29, strict, "carry 2 width") for x in w]
    out = [0] * 9
    for t in range(9):
        o = (w[t] & M29) + (kk[t - 1] if t >= 1 else 0)
        if t == 0:
            if kk[8] >> 24 and strict:
                raise ContractError("fer_mul: 24-bit multiply operand")
            o += (kk[8] & 0xFFFFFF) * R261
        out[t] = _u32(o, strict, "carry 2")
    return out


def fer_sqn(a, n, strict=True):
    for _ in range(n):
        a = fer_mul(a, a, strict)
    return a


# ---- pt_r16.h: one parallel carry round ----
def r4_carry(x, strict=True):
    k = [v >> 29 for v in x]
    out = [(x[t] & M29) + (k[t - 1] if t >= 1 else 0) for t in range(9)]
    out[0] += k[8] * R261
    return out


def r4_addn(a, b, strict=True):
    return r4_carry(add(a, b, strict), strict)


def r4_sub(a, b, strict=True):
    return r4_carry(_sub_raw(a, b, strict, "r4::sub"), strict)


# ---- tables.h: a precomp entry as stored (7 quads, or 8 with the batch path's padding) ----
def precomp_to_quads(ypx, ymx, xy2d, quads=7):
    """The 4 * quads words precomp_to_quads writes for the limb vectors (y+x, y-x, 2dxy)."""
    w = list(ypx) + list(ymx) + list(xy2d)
    assert len(w) == 27 and quads >= 7
    return w + [0] * (4 * quads - 27)


def quads_to_precomp(words):
    """The inverse (quads_to_precomp): the stored words of one entry -> the three limb vectors.
    The words past the 27th are padding and must be zero."""
    w = [int(x) for x in words]
    assert len(w) >= 28 and len(w) % 4 == 0 and not any(w[27:]), "not a precomp row"
    return w[0:9], w[9:18], w[18:27]
