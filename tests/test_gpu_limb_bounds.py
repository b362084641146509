"""The limb-bound contract of fe25519.h (N: limbs < 2^29 + 2^23, A: < 2^30 + 2^24), at its
edges, in all three forms: one lane (fe25519.h), four lanes (fe_q4.h) and one 16-lane row
(fe_r16.h, pt_r16.h) per element. The production functions run on RAW limbs (selftest ops >= 64).

The reference is Python big integers: the value of a limb vector is sum(limb_i 2^(29 i)), and a
result is right when its canonical words are that value put through the operation, mod p. The
documented output bound is asserted on the raw result limbs. oracle/fe_limbs.py is a word-exact
model of the same code that raises when a 32- or 64-bit quantity would wrap; every input is put
through it first, so it is known to be inside the contract before the GPU's result is judged
(inputs beyond a documented bound are examined in the model only, never on the GPU).

Each GPU test prints the largest output limb it saw against the bound ("MAXLIMB" lines, pytest -s).
"""
import functools
import random

import numpy as np
import pytest

import fe_limbs as F

gpu = pytest.mark.gpu
P = F.P
NB, AB = F.N_BOUND, F.A_BOUND
OP_MUL, OP_SQ, OP_MUL_SMALL, OP_ADD, OP_ADDN, OP_SUB, OP_NEG, OP_NORM, OP_CANON = 64, 65, 66, 67, 68, 69, 70, 71, 72
OP_SQN, OP_INV, OP_Q_MUL, OP_Q_SQN, OP_R_MUL, OP_R_SQN, OP_R4_CARRY, OP_R4_ADDN, OP_R4_SUB = 73, 74, 75, 76, 77, 78, 79, 80, 81
R16_BOUND = 2**29 + 2**16  # fe_r16.h: fer_mul's output
R4_BOUND0, R4_BOUND = 2**29 + 7 * 1216, 2**29 + 7  # pt_r16.h carry: lane 0, lanes 1..8


# ---------------------------------------------------------------- inputs
def edge_vectors(bound):
    """Limb vectors below `bound` (exclusive) where carries and column sums are extreme."""
    m = bound - 1
    out = [[m] * 9, [F.M29] * 9, [0] * 9, [1] + [0] * 8, [0] * 8 + [m], [0] * 8 + [F.M29]]
    for i in range(9):
        out.append([m if j == i else 0 for j in range(9)])
        out.append([m if j == i else F.M29 for j in range(9)])
    return out


def random_vector(r, bound):
    pick = (0, 1, F.M29, 1 << 29, bound - 1, None)
    return [x if x is not None else r.randrange(bound) for x in (r.choice(pick) for _ in range(9))]


@functools.lru_cache(maxsize=None)
def pair_inputs(bound_a, bound_b, count, seed):
    """(a, b) limb-vector pairs: every edge of a against the extreme vectors of b and the other
    way round, then `count` drawn pairs."""
    r = random.Random(seed)
    ea, eb = edge_vectors(bound_a), edge_vectors(bound_b)
    out = [(a, b) for a in ea for b in eb[:6]] + [(a, b) for a in ea[:6] for b in eb[6:]]
    out += [(random_vector(r, bound_a), random_vector(r, bound_b)) for _ in range(count)]
    return out


@functools.lru_cache(maxsize=None)
def mixed_pairs(count=1200, seed=11):
    """Pairs for the functions that take N or A operands on both sides: N x N, A x A, A x N, N x A."""
    out = []
    for k, (ba, bb) in enumerate([(NB, NB), (AB, AB), (AB, NB), (NB, AB)]):
        out += pair_inputs(ba, bb, count // 4, seed + k)
    return out


def rows(items, param=0, copies=1):
    """64-word input rows: operands a, b as raw limbs in words 0..17, the parameter in word 36;
    each row `copies` times in a row (the quad and row forms need whole quads / rows alike)."""
    w = np.zeros((len(items), 64), dtype=np.uint32)
    for k, (a, b) in enumerate(items):
        w[k, 0:9] = a
        w[k, 9:18] = b
    w[:, 36] = param
    return np.repeat(w, copies, axis=0) if copies > 1 else w


def words_value(ws):
    return sum(int(x) << (32 * i) for i, x in enumerate(ws))


MAXLIMB = {}


def check(engine, name, op, items, want, model, bound, param=0, copies=1, bound0=None):
    """Runs `op` on items; asserts the value (want(a, b) mod p) on the canonical words and on the
    raw limbs, the output bound on the raw limbs (bound0: limb 0's own bound), and that every copy
    of a row agrees. model(a, b) runs first: it raises if the input leaves the contract, and its
    limbs must be the GPU's wherever the model is of the same form."""
    params = param if isinstance(param, (list, tuple)) else [param] * len(items)
    w = rows(items, 0, copies)
    w[:, 36] = np.repeat(np.array(params, dtype=np.uint32), copies)
    expect = [model(a, b, c) for (a, b), c in zip(items, params)]  # ContractError: a bad test input
    out = engine.selftest(op, w)
    if copies > 1:
        first = np.repeat(out[::copies], copies, axis=0)
        assert (out == first).all(), f"{name}: the lanes of one element disagree"
        out = out[::copies]
    big = 0
    for (a, b), c, o, m in zip(items, params, out, expect):
        limbs = [int(x) for x in o[:9]]
        v = want(a, b, c) % P
        assert words_value(o[40:48]) == v, (name, a, b, c)
        assert F.value(limbs) % P == v, (name, "raw limbs", a, b, c)
        assert limbs == m, (name, "model limbs", a, b, c)
        assert limbs[0] < (bound0 or bound) and max(limbs[1:]) < bound, (name, "bound", a, b, limbs)
        big = max(big, max(limbs))
    MAXLIMB[name] = big
    print(f"MAXLIMB {name}: {big:#x} = 2^29 + {big - 2**29} (bound {bound:#x})")


# ---------------------------------------------------------------- the model against big integers (CPU)
def test_model_matches_big_integers():
    """The model itself: products, squares, sums and differences of extreme and drawn vectors are
    the big-integer results, no column or carry wraps for N or A operands, outputs are N."""
    for a, b in mixed_pairs():
        va, vb = F.value(a), F.value(b)
        for f, g in [(F.mul, va * vb), (F.feq_mul, va * vb), (F.fer_mul, va * vb), (F.sub, va - vb),
                     (F.addn, va + vb), (F.r4_addn, va + vb), (F.r4_sub, va - vb)]:
            r = f(a, b)
            assert F.value(r) % P == g % P and max(r) < NB, (f.__name__, a, b)
        assert F.value(F.sq(a)) % P == va * va % P
        assert F.value(F.canon(a)) == va % P and F.to_words(a) == [(va % P >> 32 * j) & F.U32 for j in range(8)]
        assert F.eq(a, b) == ((va - vb) % P == 0)


def test_model_fe_normalize_true_input_bound():
    """fe_normalize's serial carry: every limb 2^32 - 8 is the largest input that does not wrap
    (each limb takes a carry of at most 7); 2^32 - 1 in limb 0 under a limb 1 of 2^32 - 7 wraps.
    The one parallel round of pt_r16.h's carry cannot wrap for any 32-bit limbs."""
    top = [F.NORM_IN_MAX] * 9
    assert F.value(F.normalize(top)) % P == F.value(top) % P
    bad = [F.U32, F.NORM_IN_MAX + 1] + [0] * 7
    with pytest.raises(F.ContractError):
        F.normalize(bad)
    assert F.value(F.normalize(bad, strict=False)) % P != F.value(bad) % P
    # the largest limb a call site hands it: fe_sub's a + (bias - b) with a an A value
    assert AB - 1 + max(F.SUB_BIAS) < F.NORM_IN_MAX
    full = [F.U32] * 9
    r = F.r4_carry(full)
    assert F.value(r) % P == F.value(full) % P and r[0] < R4_BOUND0 and max(r[1:]) < R4_BOUND


def test_model_headroom_of_an_unnormalised_sum():
    """What the bounds protect: A x A keeps every column below 2^64 (9 (2^30 + 2^24)^2 < 2^63.3),
    and twice that bound on one side does not."""
    F.mul([AB - 1] * 9, [AB - 1] * 9)
    # An addition's rZ = 2 ZZ + TT left unnormalised (fe_add for fe_addn) is outside the contract:
    # limbs up to 3 (2^29 + 2^17) > A. Its only uses are products with an N or an A value, and
    # even with every limb at that maximum no column wraps in any of the three forms (column sums
    # grow with the limbs, so this case bounds all): the result stays right, and only a bound
    # check on the p1p1 limbs (test_gpu_points.py) can notice a dropped normalisation there.
    lazy3 = [3 * (2**29 + 2**17)] * 9
    assert max(lazy3) >= AB
    for f in (F.mul, F.feq_mul, F.fer_mul):
        r = f(lazy3, [AB - 1] * 9)
        assert F.value(r) % P == F.value(lazy3) * F.value([AB - 1] * 9) % P and max(r) < NB
    with pytest.raises(F.ContractError):
        F.mul([2 * AB] * 9, [AB - 1] * 9)
    with pytest.raises(F.ContractError):
        F.sub([0] * 9, [F.SUB_BIAS[1] + 1] * 9)


def test_model_fe_canon_folds():
    """fe_canon after one fold of the bits >= 255: the value is < 2^255 + 2^30 < 2 p, which the
    final conditional subtraction of p completes, so for inputs inside the contract the second
    fold changes no result (a test cannot tell the two apart); with no fold at all the multiples
    of p from 2 p on are missed."""
    vecs = canon_vectors()
    assert all(F.canon(a, folds=1) == F.canon(a) for a in vecs)
    assert any(F.canon(a, folds=0) != F.canon(a) for a in vecs)


# ---------------------------------------------------------------- one lane per element
@gpu
def test_fe_mul_sq_lazy_operands(engine):
    items = mixed_pairs()
    check(engine, "fe_mul", OP_MUL, items, lambda a, b, c: F.value(a) * F.value(b), lambda a, b, c: F.mul(a, b), NB)
    check(engine, "fe_sq", OP_SQ, items, lambda a, b, c: F.value(a) ** 2, lambda a, b, c: F.sq(a), NB)


@gpu
def test_fe_mul_small_lazy_operand(engine):
    r = random.Random(12)
    items = mixed_pairs()
    cs = [r.choice((0, 1, 2**26 - 1, 121666, r.randrange(2**26))) for _ in items]
    cs[0] = 2**26 - 1  # every limb at the A maximum times the largest constant
    check(engine, "fe_mul_small", OP_MUL_SMALL, items, lambda a, b, c: F.value(a) * c,
          lambda a, b, c: F.mul_small(a, c), NB, param=cs)


@gpu
def test_fe_sub_lazy_operands(engine):
    """fe_sub takes N or A on both sides (the sibling of test_fe_sub_tight_inputs); fe_neg likewise."""
    items = mixed_pairs()
    check(engine, "fe_sub", OP_SUB, items, lambda a, b, c: F.value(a) - F.value(b), lambda a, b, c: F.sub(a, b), NB)
    check(engine, "fe_neg", OP_NEG, items, lambda a, b, c: -F.value(a), lambda a, b, c: F.neg(a), NB)


@gpu
def test_fe_add_addn(engine):
    """fe_add: N + N -> A, unnormalised; fe_addn: (N|A) + (N|A) -> N."""
    nn = pair_inputs(NB, NB, 600, 13)
    check(engine, "fe_add", OP_ADD, nn, lambda a, b, c: F.value(a) + F.value(b), lambda a, b, c: F.add(a, b), AB)
    check(engine, "fe_addn", OP_ADDN, mixed_pairs(), lambda a, b, c: F.value(a) + F.value(b),
          lambda a, b, c: F.addn(a, b), NB)


@gpu
def test_fe_normalize_at_its_bound(engine):
    """Every limb 2^32 - 8, the largest input the serial carry takes without a wrap, its edges
    and drawn vectors below it."""
    r = random.Random(14)
    bound = F.NORM_IN_MAX + 1
    vs = edge_vectors(bound) + [random_vector(r, bound) for _ in range(1500)]
    items = [(v, [0] * 9) for v in vs]
    check(engine, "fe_normalize", OP_NORM, items, lambda a, b, c: F.value(a), lambda a, b, c: F.normalize(a), NB)


@gpu
def test_fe_sqn_invert_lazy_operand(engine):
    r = random.Random(15)
    vs = edge_vectors(AB) + edge_vectors(NB) + [random_vector(r, AB) for _ in range(300)]
    items = [(v, [0] * 9) for v in vs]
    check(engine, "fe_sqn", OP_SQN, items, lambda a, b, c: pow(F.value(a), 2**30, P),
          lambda a, b, c: F.sqn(a, 30), NB, param=30)
    items = items[::3]  # (the model of an inversion is 265 products)
    out = engine.selftest(OP_INV, rows(items))
    for (a, _), o in zip(items, out):
        assert words_value(o[40:48]) == pow(F.value(a), P - 2, P), a
        assert max(int(x) for x in o[:9]) < NB


# ---------------------------------------------------------------- fe_canon and the predicates
@functools.lru_cache(maxsize=None)
def canon_vectors():
    """Lazy representations of 0 and p - 1, the values around 2^255 and 2^261, and vectors whose
    first fold's carry runs through limbs 0..7 into limb 8. All within the A bound."""
    vals = []
    for k in (1, 2, 63, 64):
        vals += [k * P, k * P - 1, k * P + 1]
    vals += [P - 1, P + 1, 2**255, 2**255 - 1, 2**261 - 1216, 2**261 - 1215, 2**261 - 1217, 2**261 - 1, 0, 1,
             2**256 - 1, 2**256 - 38, 2**256 - 39]
    # q 2^255 + (2^255 - 1 - j): after the first fold adds 19 q, limbs 0..7 overflow into limb 8
    for q in (1, 2, 31, 63):
        for j in (0, 1, 18, 19 * q - 1, 19 * q, 19 * q + 1):
            if q * 2**255 + 2**255 - 1 - j < 2**261:
                vals.append(q * 2**255 + 2**255 - 1 - j)
    vecs = []
    for v in vals:
        t = F.tight(v)
        vecs += [t, F.borrowed(t)]
    # the largest multiples of p (and their predecessors) that fit the A bound at all
    kmax = (AB - 1) * F.value([1] * 9) // P
    found = 0
    for k in range(kmax, 0, -1):
        g, g1 = F.greedy(k * P, AB), F.greedy(k * P - 1, AB)
        if g is not None and g1 is not None:
            vecs += [g, g1]
            found += 1
            if found == 3:
                break
    assert found == 3 and k >= 128
    r = random.Random(16)
    vecs += edge_vectors(AB) + edge_vectors(NB) + [random_vector(r, AB) for _ in range(1500)]
    assert all(max(v) < AB for v in vecs)
    return vecs


@gpu
def test_fe_canon_and_predicates(engine):
    """fe_canon gives the canonical limbs of the value; fe_is_zero holds for exactly the multiples
    of p, fe_is_negative is the parity of the canonical value, fe_eq compares values; fe_to_words
    of the lazy input is the canonical value."""
    r = random.Random(17)
    vecs = canon_vectors()
    items = []
    for k, a in enumerate(vecs):
        va = F.value(a)
        other = r.choice((0, 1, 2))
        vb = (va + r.choice((0, 0, 1, P, P - 1))) if other else F.value(vecs[k - 1])
        b = F.tight(vb % 2**261) if other < 2 else (F.greedy(vb, AB) or F.tight(vb % 2**261))
        items.append((a, b))
    for a, b in items:
        F.canon(a), F.eq(a, b)  # inside the contract
    out = engine.selftest(OP_CANON, rows(items))
    zeros = 0
    for (a, b), o in zip(items, out):
        va, vb = F.value(a), F.value(b)
        assert [int(x) for x in o[:9]] == F.tight(va % P), ("fe_canon", a)
        assert words_value(o[40:48]) == va % P, ("fe_to_words", a)
        fl = int(o[36])
        assert bool(fl & 1) == (va % P == 0), ("fe_is_zero", a)
        assert bool(fl & 2) == bool(va % P & 1), ("fe_is_negative", a)
        assert bool(fl & 4) == ((va - vb) % P == 0), ("fe_eq", a, b)
        zeros += va % P == 0
    assert zeros >= 15  # the multiples of p are really among the inputs


# ---------------------------------------------------------------- four lanes / one row per element
@gpu
def test_quad_form_lazy_operands(engine):
    items = mixed_pairs()
    check(engine, "feq_mul", OP_Q_MUL, items, lambda a, b, c: F.value(a) * F.value(b),
          lambda a, b, c: F.feq_mul(a, b), NB, copies=4)
    items = items[::8]
    check(engine, "feq_sqn", OP_Q_SQN, items, lambda a, b, c: pow(F.value(a), 2**30, P),
          lambda a, b, c: F.feq_sqn(a, 30), NB, param=30, copies=4)


@gpu
def test_row_form_lazy_operands(engine):
    items = mixed_pairs()
    check(engine, "fer_mul", OP_R_MUL, items, lambda a, b, c: F.value(a) * F.value(b),
          lambda a, b, c: F.fer_mul(a, b), R16_BOUND, copies=16)
    items = items[::8]
    check(engine, "fer_sqn", OP_R_SQN, items, lambda a, b, c: pow(F.value(a), 2**30, P),
          lambda a, b, c: F.fer_sqn(a, 30), R16_BOUND, param=30, copies=16)


@gpu
def test_row_form_carry_addn_sub(engine):
    """pt_r16.h: one parallel carry round takes any 32-bit limbs to lane 0 < 2^29 + 7 * 1216 and
    lanes 1..8 < 2^29 + 8; addn and sub on N or A operands."""
    r = random.Random(18)
    vs = edge_vectors(2**32) + [random_vector(r, 2**32) for _ in range(600)]
    check(engine, "r4::carry", OP_R4_CARRY, [(v, [0] * 9) for v in vs], lambda a, b, c: F.value(a),
          lambda a, b, c: F.r4_carry(a), R4_BOUND, copies=16, bound0=R4_BOUND0)
    items = mixed_pairs()
    check(engine, "r4::addn", OP_R4_ADDN, items, lambda a, b, c: F.value(a) + F.value(b),
          lambda a, b, c: F.r4_addn(a, b), R4_BOUND, copies=16, bound0=R4_BOUND0)
    check(engine, "r4::sub", OP_R4_SUB, items, lambda a, b, c: F.value(a) - F.value(b),
          lambda a, b, c: F.r4_sub(a, b), R4_BOUND, copies=16, bound0=R4_BOUND0)


@gpu
def test_three_forms_agree(engine):
    """fe_mul, feq_mul and fer_mul give the same residue for the same lazy operands (their limbs
    may differ: canonical words are compared)."""
    items = mixed_pairs()
    one = engine.selftest(OP_MUL, rows(items))[:, 40:48]
    quad = engine.selftest(OP_Q_MUL, rows(items, copies=4))[::4, 40:48]
    row = engine.selftest(OP_R_MUL, rows(items, copies=16))[::16, 40:48]
    assert (one == quad).all() and (one == row).all()
