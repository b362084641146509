"""fe_mul / fe_sq / fe_sqn (fe25519.h) limb for limb against the order of summation they had
before the carry went through the MAD addend.

fe_reduce_scan now builds each low column as one v_mad_u64_u32 chain that starts from the previous
column's carry. The model below is the earlier order, written out here: every column summed on its
own, the high columns folded into the low sums (L * 1216 -> column k - 9, H * 9728 -> column
k - 8), then the ripple lo[k + 1] += lo[k] >> 29. Both orders add the same non-negative integers,
so a low sum after its ripple step IS the new order's finished chain of that column, and every
partial sum of either order is at most that value: the model asserts it stays below 2^64 (the
bound the header documents: 2^63.3 + 2^44.6 + 2^42.3 + 2^35), and the GPU's raw limbs (selftest
ops 64, 65, 73 take and return unmasked limbs) must be the model's, all 9 of them.

Inputs: every limb at the A maximum 2^30 + 2^24 - 1 and at the N maximum 2^29 + 2^23 - 1, each
single limb at either maximum with the others zero (the largest single carries), lazy forms of 0
and p - 1 (multiples of p added, limbs borrowed from their neighbours), and 256 drawn N values,
each on the 64 lanes of a wave.
"""
import functools
import random

import numpy as np
import pytest

gpu = pytest.mark.gpu
P = 2**255 - 19
M29 = (1 << 29) - 1
R261 = 1216
N_MAX = 2**29 + 2**23 - 1
A_MAX = 2**30 + 2**24 - 1
OP_MUL, OP_SQ, OP_SQN = 64, 65, 73


# ---------------------------------------------------------------- the model (earlier order)
def value(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def u64(x, what):
    assert 0 <= x < 1 << 64, f"{what} wraps 64 bits: {x:#x}"
    return x


def reduce_columns(cols):
    """17 column sums -> 9 limbs: fold the high columns, ripple, top fold."""
    lo = [u64(c, "column") for c in cols[:9]]
    for k in range(9, 17):
        c = u64(cols[k], "high column")
        lo[k - 9] = u64(lo[k - 9] + (c & 0xFFFFFFFF) * R261, "low sum")
        lo[k - 8] = u64(lo[k - 8] + (c >> 32) * (8 * R261), "low sum")
    r = [0] * 9
    for k in range(8):
        r[k] = lo[k] & M29
        lo[k + 1] = u64(lo[k + 1] + (lo[k] >> 29), "chain")  # = the new order's chain of column k + 1
    r[8] = lo[8] & M29
    t0 = r[0] + (lo[8] >> 29) * R261
    assert t0 < 1 << 64
    r[0] = t0 & M29
    r[1] += t0 >> 29
    assert r[1] < 1 << 32
    return r


def model_mul(a, b):
    cols = [sum(a[i] * b[k - i] for i in range(max(0, k - 8), min(k, 8) + 1)) for k in range(17)]
    return reduce_columns(cols)


def model_sq(a):
    a2 = [(x << 1) & 0xFFFFFFFF for x in a]
    assert all(y == 2 * x for x, y in zip(a, a2)), "2a wraps 32 bits"
    cols = []
    for k in range(17):
        c = 0 if k & 1 else a[k >> 1] * a[k >> 1]
        c += sum(a2[i] * a[k - i] for i in range(max(0, k - 8), 9) if i < k - i)
        cols.append(c)
    return reduce_columns(cols)


def model_sqn(a, n):
    for _ in range(n):
        a = model_sq(a)
    return a


# ---------------------------------------------------------------- inputs
def tight(v):
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & M29 for i in range(9)]


def borrowed(limbs):
    """The same value with 2^29 moved from every limb that has one to spare into the limb below."""
    out = list(limbs)
    for i in range(8):
        if out[i + 1] >= 1:
            out[i + 1] -= 1
            out[i] += 1 << 29
    return out


@functools.lru_cache(maxsize=None)
def edge_vectors():
    out = [[A_MAX] * 9, [N_MAX] * 9]
    for m in (A_MAX, N_MAX):
        out += [[m if j == i else 0 for j in range(9)] for i in range(9)]
    for k in (0, 1, 2, 63):  # 64 p = 2^261 - 1216: every k p + (p - 1) here is below 2^261
        for v in (k * P, k * P + P - 1):
            out.append(tight(v))
            out.append(borrowed(tight(v)))
    assert all(max(v) <= A_MAX for v in out)
    return out


@functools.lru_cache(maxsize=None)
def drawn_vectors():
    r = random.Random(2029)
    pick = (0, 1, M29, 1 << 29, N_MAX, None, None, None)
    return [[x if x is not None else r.randrange(N_MAX + 1) for x in (r.choice(pick) for _ in range(9))]
            for _ in range(256)]


@functools.lru_cache(maxsize=None)
def pairs(which):
    """(a, b) items: edges against themselves and against their neighbour in the list (so all-A
    meets all-A, and all-A meets all-N), drawn values against the next drawn value."""
    vs = edge_vectors() if which == "edge" else drawn_vectors()
    out = [(v, vs[(i + 1) % len(vs)]) for i, v in enumerate(vs)]
    if which == "edge":
        out += [(v, v) for v in vs]
    return out


@functools.lru_cache(maxsize=None)
def expected(op, which, n=0):
    """The model's limbs for every item, computed once per (op, inputs)."""
    if op == OP_MUL:
        return [model_mul(a, b) for a, b in pairs(which)]
    return [model_sqn(a, n) for a, _ in pairs(which)]


def rows(items, param, copies):
    w = np.zeros((len(items), 64), dtype=np.uint32)
    for k, (a, b) in enumerate(items):
        w[k, 0:9] = a
        w[k, 9:18] = b
    w[:, 36] = param
    return np.repeat(w, copies, axis=0) if copies > 1 else w


def run(engine, op, which, n=0):
    items = pairs(which)
    copies = 64 if which == "drawn" else 1  # a drawn value fills a wave
    out = engine.selftest(op, rows(items, n, copies))
    if copies > 1:
        assert (out == np.repeat(out[::copies], copies, axis=0)).all(), "the lanes of one wave disagree"
        out = out[::copies]
    want = expected(op, which, n)
    for (a, b), o, m in zip(items, out, want):
        assert [int(x) for x in o[:9]] == m, (op, n, a, b)


# ---------------------------------------------------------------- CPU: the model itself
def test_model_is_multiplication_mod_p():
    """The earlier order's model against plain big-integer products mod p, over the GPU tests' own
    inputs: no column, low sum or chain wraps (asserted inside the model), outputs are N."""
    for which in ("edge", "drawn"):
        for (a, b), r in zip(pairs(which), expected(OP_MUL, which)):
            assert value(r) % P == value(a) * value(b) % P and max(r) <= N_MAX, (a, b)
        for n in (1, 2, 50):
            for (a, _), r in zip(pairs(which), expected(OP_SQN, which, n)):
                assert value(r) % P == pow(value(a), 2**n, P) and max(r) <= N_MAX, (n, a)


def test_model_chain_bound_is_tight_enough():
    """The documented chain bound at its worst input, every limb at the A maximum on both sides:
    a finished chain is below 2^63.3 + 2^44.6 + 2^42.3 + 2^35 < 2^64, and one more A-sized
    operand bit would not fit (the model raises)."""
    model_mul([A_MAX] * 9, [A_MAX] * 9)
    with pytest.raises(AssertionError):
        model_mul([2 * A_MAX] * 9, [A_MAX] * 9)


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("which", ["edge", "drawn"])
def test_fe_mul_limbs(engine, which):
    run(engine, OP_MUL, which)


@gpu
@pytest.mark.parametrize("which", ["edge", "drawn"])
def test_fe_sq_limbs(engine, which):
    run(engine, OP_SQ, which, 1)


@gpu
@pytest.mark.parametrize("n", [1, 2, 50])
@pytest.mark.parametrize("which", ["edge", "drawn"])
def test_fe_sqn_limbs(engine, which, n):
    run(engine, OP_SQN, which, n)
