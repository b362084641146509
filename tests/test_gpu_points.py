"""Point operations by themselves, in all three forms: one lane per point (ge25519.h: p2_dbl,
p3_add_cached, p3_add_precomp, cached_cneg, precomp_cneg, p3_neg), four lanes per point
(quad25519.h: qp_dbl, qp_add, qp_in_torsion) and one wave per point (pt_r16.h: dbl, addp), run
through the raw-limb selftest ops (>= 96) on chosen operands.

Points come in two ways. As 32-byte encodings: the reference is oracle/zip215.py (decompress,
add, scalarmult, compress), over the small-order encodings (non-canonical ones included), B,
multiples of B, B plus each torsion point, and drawn valid encodings: 2P, P + Q for all pairs of
the edge set (Q = P, Q = -P, either operand the identity, torsion + torsion among them), negated
table entries, and additions after 1, 3 and 16 doublings (Z != 1 operands). As raw extended
coordinates with limbs at the N maximum (not on the curve): every output coordinate is checked
against the same formula (dbl-2008-hwcd; the HWCD unified addition) in big integers, and against
the limb bound ge25519.h documents (p3 coordinates N; p1p1 N or A; cached.YpX A).
"""
import functools
import random

import numpy as np
import pytest

import fe_limbs as F
import zip215 as Z

pytestmark = pytest.mark.gpu
P = Z.P
NB, AB = F.N_BOUND, F.A_BOUND
OP_DBL, OP_ADD_CACHED, OP_ADD_PRECOMP, OP_Q_DBL, OP_Q_ADD, OP_Q_TORSION, OP_R_DBL, OP_R_ADD = 96, 97, 98, 99, 100, 101, 102, 103
DBL_FORMS = [(OP_DBL, 1), (OP_Q_DBL, 4), (OP_R_DBL, 64)]  # (op, lanes per point)
ADD_FORMS = [(OP_ADD_CACHED, 1), (OP_ADD_PRECOMP, 1), (OP_Q_ADD, 4), (OP_R_ADD, 64)]
QSELF, QSWAP, NEG, RAW, QNEG, P1P1 = 1 << 8, 2 << 8, 1 << 10, 1 << 11, 1 << 12, 1 << 13
# bound on a result coordinate's limbs by lanes per point: N; fe_r16.h states 2^29 + 2^16 for its products
FORM_BOUND = {1: NB, 4: NB, 64: 2**29 + 2**16}


@functools.lru_cache(maxsize=None)
def torsion_encodings():
    return [e for e, _ in Z.small_order_encodings()]


@functools.lru_cache(maxsize=None)
def edge_encodings():
    """Small-order encodings (canonical and not), B, multiples of B (-B among them), B + torsion."""
    encs = list(torsion_encodings())
    for k in (1, 2, 3, 5, Z.L - 1, Z.L - 2):
        encs.append(Z.compress(Z.scalarmult(Z.B_POINT, k)))
    for t in Z.torsion_points().values():
        encs.append(Z.compress(Z.add(Z.B_POINT, t)))
    return encs


@functools.lru_cache(maxsize=None)
def random_encodings(count=300, seed=21):
    r = random.Random(seed)
    out = []
    while len(out) < count:
        e = r.randrange(2**256).to_bytes(32, "little")
        if Z.decompress(e) is not None:
            out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def edge_pairs():
    e = edge_encodings()
    return [(a, b) for a in e for b in e]


@functools.lru_cache(maxsize=None)
def random_pairs():
    e = random_encodings()
    return [(a, e[(i * 7 + 1) % len(e)]) for i, a in enumerate(e)] + [(a, a) for a in e[:20]]


@functools.lru_cache(maxsize=None)
def reference_sums(which, kdbl, negate):
    """compress((2^kdbl P) +- Q) for the pairs of the edge set ('edge') or the drawn ones, once."""
    pairs = edge_pairs() if which == "edge" else random_pairs()
    dec = {e: Z.decompress(e) for pr in pairs for e in pr}
    out = []
    for a, b in pairs:
        p, q = dec[a], dec[b]
        for _ in range(kdbl):
            p = Z.double(p)
        s = Z.add(p, Z.neg(q) if negate else q)
        out.append((Z.compress(s), Z.is_identity(s)))
    return out


def enc_rows(pairs, param, copies):
    w = np.zeros((len(pairs), 64), dtype=np.uint32)
    for k, (a, b) in enumerate(pairs):
        w[k, 40:48] = np.frombuffer(a, dtype=np.uint32)
        w[k, 48:56] = np.frombuffer(b, dtype=np.uint32)
    w[:, 36] = param
    return np.repeat(w, copies, axis=0) if copies > 1 else w


def run(engine, op, w, copies):
    out = engine.selftest(op, w)
    if copies > 1:
        assert (out == np.repeat(out[::copies], copies, axis=0)).all(), (op, "the lanes of one point disagree")
        out = out[::copies]
    return out


def coords(o):
    return [[int(x) for x in o[9 * c:9 * c + 9]] for c in range(4)]


def check_point_rows(op, out, pairs, want, bound):
    """The compressed result and the identity flag against the reference; the raw extended
    coordinates are consistent (T Z = X Y: the next addition uses T) and within the bound."""
    for pr, o, (enc, ident) in zip(pairs, out, want):
        assert int(o[36]) & 6 == 6, (op, "decode", pr)
        assert o[40:48].astype("<u4").tobytes() == enc, (op, pr[0].hex(), pr[1].hex())
        assert bool(int(o[36]) & 1) == ident, (op, "p3_is_identity", pr[0].hex(), pr[1].hex())
        X, Y, Zc, T = coords(o)
        assert (F.value(T) * F.value(Zc) - F.value(X) * F.value(Y)) % P == 0, (op, "T", pr)
        assert max(max(c) for c in (X, Y, Zc, T)) < bound, (op, "bound", pr)


# ---------------------------------------------------------------- points through encodings
@pytest.mark.parametrize("op,copies", DBL_FORMS)
def test_double(engine, op, copies):
    encs = edge_encodings() + random_encodings()
    pairs = [(e, e) for e in encs]
    want = []
    for e in encs:
        d = Z.double(Z.decompress(e))
        want.append((Z.compress(d), Z.is_identity(d)))
    out = run(engine, op, enc_rows(pairs, 0, copies), copies)
    check_point_rows(op, out, pairs, want, FORM_BOUND[copies])


@pytest.mark.parametrize("op,copies", DBL_FORMS)
def test_eight_times_torsion_is_identity(engine, op, copies):
    """Three doublings of every small-order encoding give the identity; of B, of multiples of B
    and of B + torsion they do not."""
    encs = edge_encodings()
    pairs = [(e, e) for e in encs]
    out = run(engine, op, enc_rows(pairs, 2, copies), copies)  # two doublings first, then the op's own
    nt = len(torsion_encodings())
    for k, (e, o) in enumerate(zip(encs, out)):
        assert bool(int(o[36]) & 1) == (k < nt), e.hex()
        assert o[40:48].astype("<u4").tobytes() == Z.compress(Z.scalarmult(Z.decompress(e), 8)), e.hex()


def test_qp_in_torsion(engine):
    """qp_in_torsion agrees with "[8]P is the identity" on torsion and non-torsion points, with
    Z = 1 and after doublings (Z != 1)."""
    encs = edge_encodings() + random_encodings()[:100]
    pairs = [(e, e) for e in encs]
    for kdbl in (0, 1, 2):
        out = run(engine, OP_Q_TORSION, enc_rows(pairs, kdbl, 4), 4)
        for e, o in zip(encs, out):
            want = Z.is_identity(Z.scalarmult(Z.decompress(e), 8 << kdbl))
            assert bool(int(o[36]) & 8) == want, (kdbl, e.hex())
    assert sum(Z.is_identity(Z.scalarmult(Z.decompress(e), 8)) for e in encs) == len(torsion_encodings())


@pytest.mark.parametrize("op,copies", ADD_FORMS)
def test_add_all_edge_pairs(engine, op, copies):
    pairs = edge_pairs()
    out = run(engine, op, enc_rows(pairs, 0, copies), copies)
    check_point_rows(op, out, pairs, reference_sums("edge", 0, False), FORM_BOUND[copies])


@pytest.mark.parametrize("op,copies", ADD_FORMS)
def test_add_random_pairs(engine, op, copies):
    pairs = random_pairs()
    out = run(engine, op, enc_rows(pairs, 0, copies), copies)
    check_point_rows(op, out, pairs, reference_sums("random", 0, False), FORM_BOUND[copies])


@pytest.mark.parametrize("op,copies", ADD_FORMS)
def test_subtract_by_negated_entry(engine, op, copies):
    """P + (-Q) with the table entry negated (cached_cneg, precomp_cneg; -Q in the quad and row
    forms) is the reference's P - Q; with the flag clear it is P + Q (the other tests)."""
    for which in ("edge", "random"):
        pairs = edge_pairs() if which == "edge" else random_pairs()
        out = run(engine, op, enc_rows(pairs, NEG, copies), copies)
        check_point_rows(op, out, pairs, reference_sums(which, 0, True), FORM_BOUND[copies])


@pytest.mark.parametrize("op", [OP_ADD_CACHED, OP_ADD_PRECOMP])
def test_p3_neg_and_double_negation(engine, op):
    """p3_neg(Q) then the addition is P - Q; p3_neg and a negated entry together are P + Q."""
    pairs = edge_pairs()
    out = run(engine, op, enc_rows(pairs, QNEG, 1), 1)
    check_point_rows(op, out, pairs, reference_sums("edge", 0, True), NB)
    out = run(engine, op, enc_rows(pairs, QNEG | NEG, 1), 1)
    check_point_rows(op, out, pairs, reference_sums("edge", 0, False), NB)


@pytest.mark.parametrize("kdbl", [1, 3, 16])
@pytest.mark.parametrize("op,copies", ADD_FORMS)
def test_add_after_doublings(engine, op, copies, kdbl):
    """(2^k P) + Q: the addition's first operand has Z != 1 and was made by the kernel itself."""
    which = "edge" if copies < 64 else "random"
    pairs = edge_pairs() if which == "edge" else random_pairs()
    out = run(engine, op, enc_rows(pairs, kdbl, copies), copies)
    check_point_rows(op, out, pairs, reference_sums(which, kdbl, False), FORM_BOUND[copies])


def test_forms_agree(engine):
    """The three point forms give the same encoding for the same operands."""
    pairs = random_pairs()
    res = [run(engine, op, enc_rows(pairs, 3, c), c)[:, 40:48] for op, c in ADD_FORMS]
    assert all((r == res[0]).all() for r in res[1:])
    res = [run(engine, op, enc_rows(pairs, 3, c), c)[:, 40:48] for op, c in DBL_FORMS]
    assert all((r == res[0]).all() for r in res[1:])


# ---------------------------------------------------------------- points with lazy coordinates
@functools.lru_cache(maxsize=None)
def lazy_points(count=400, seed=31):
    """Extended coordinates (X, Y, Z, T) as raw limbs within N, extreme ones first."""
    r = random.Random(seed)
    m = NB - 1
    ext = [[m] * 9, [F.M29] * 9, [0] * 8 + [m], [m] + [0] * 8, [1] + [0] * 8, [0] * 9]
    pts = [(ext[0],) * 4, (ext[1],) * 4]
    pts += [tuple(ext[(i + j) % len(ext)] for j in range(4)) for i in range(len(ext))]
    for i in range(9):
        v = [m if j == i else F.M29 for j in range(9)]
        pts.append((v, ext[0], v, ext[0]))
    draw = lambda: [r.choice((0, 1, F.M29, 1 << 29, m, r.randrange(NB))) for _ in range(9)]
    pts += [(draw(), draw(), draw(), draw()) for _ in range(count)]
    return pts


def raw_rows(pts, param, copies, q_enc=None):
    w = np.zeros((len(pts), 64), dtype=np.uint32)
    for k, pt in enumerate(pts):
        for c in range(4):
            w[k, 9 * c:9 * c + 9] = pt[c]
    if q_enc is not None:
        w[:, 48:56] = np.frombuffer(q_enc, dtype=np.uint32)
    w[:, 36] = param | RAW
    return np.repeat(w, copies, axis=0) if copies > 1 else w


def dbl_p1p1(X, Y, Zc):
    XX, YY, ZZ, S2 = X * X, Y * Y, Zc * Zc, (X + Y) ** 2
    rY, rZ = YY + XX, YY - XX
    return S2 - rY, rY, rZ, 2 * ZZ - rZ  # (X, Y, Z, T) of the completed point


def add_p1p1(p, q, negate=False, precomp=False):
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    ypx, ymx, t2d = Y2 + X2, Y2 - X2, T2 * Z.D2
    if negate:
        ypx, ymx, t2d = ymx, ypx, -t2d
    PP, MM, TT = (Y1 + X1) * ypx, (Y1 - X1) * ymx, T1 * t2d
    ZZ2 = 2 * Z1 if precomp else 2 * Z1 * Z2
    return PP - MM, PP + MM, ZZ2 + TT, ZZ2 - TT


def to_p3(c):
    X, Y, Zc, T = c
    return X * T, Y * Zc, Zc * T, X * Y


def q_of(p, mode):
    return p if mode == QSELF else (p[1], p[0], p[3], p[2])


MAXLIMB = {}


def check_coords(name, out, want, bounds):
    big = 0
    for k, (o, w) in enumerate(zip(out, want)):
        got = coords(o)
        for c in range(4):
            assert F.value(got[c]) % P == w[c] % P, (name, k, "XYZT"[c])
            assert max(got[c]) < bounds[c], (name, k, "XYZT"[c], "bound")
            big = max(big, max(got[c]))
    MAXLIMB[name] = big
    print(f"MAXLIMB {name}: {big:#x} (bounds {[hex(b) for b in bounds]})")


@pytest.mark.parametrize("op,copies", DBL_FORMS)
def test_lazy_double(engine, op, copies):
    pts = lazy_points()
    vals = [tuple(F.value(c) for c in pt) for pt in pts]
    out = run(engine, op, raw_rows(pts, 0, copies), copies)
    check_coords(f"dbl[{op}]", out, [to_p3(dbl_p1p1(*v[:3])) for v in vals], [FORM_BOUND[copies]] * 4)
    if op == OP_DBL:  # the completed point: X, Z, T normalised, Y a lazy sum
        out = run(engine, op, raw_rows(pts, P1P1, 1), 1)
        check_coords("p2_dbl p1p1", out, [dbl_p1p1(*v[:3]) for v in vals], [NB, AB, NB, NB])


@pytest.mark.parametrize("mode", [QSELF, QSWAP])
@pytest.mark.parametrize("op,copies", [(OP_ADD_CACHED, 1), (OP_Q_ADD, 4), (OP_R_ADD, 64)])
def test_lazy_add(engine, op, copies, mode):
    """Both operands lazy: Q is P itself or P's (Y, X, T, Z); with and without a negated entry."""
    pts = lazy_points()
    vals = [tuple(F.value(c) for c in pt) for pt in pts]
    for neg in (0, NEG):
        want = [add_p1p1(v, q_of(v, mode), bool(neg)) for v in vals]
        out = run(engine, op, raw_rows(pts, mode | neg, copies), copies)
        check_coords(f"add[{op}]", out, [to_p3(w) for w in want], [FORM_BOUND[copies]] * 4)
        if op == OP_ADD_CACHED:
            for pt, o in zip(pts, out):  # cached(Q).YpX as used: a lazy sum (or Y - X when negated)
                q = q_of(pt, mode)
                ypx = [int(x) for x in o[48:57]]
                assert max(ypx) < AB and F.value(ypx) % P == (F.value(q[1]) + (-1 if neg else 1) * F.value(q[0])) % P
            out = run(engine, op, raw_rows(pts, mode | neg | P1P1, 1), 1)
            check_coords("p3_add_cached p1p1", out, want, [NB, AB, NB, NB])


def test_lazy_add_precomp(engine):
    """A lazy first operand against a Z = 1 table entry (B, and a small-order point)."""
    pts = lazy_points()
    vals = [tuple(F.value(c) for c in pt) for pt in pts]
    for q_enc in (Z.compress(Z.B_POINT), torsion_encodings()[-1]):
        q = Z.decompress(q_enc)
        for neg in (0, NEG):
            want = [add_p1p1(v, q, bool(neg), precomp=True) for v in vals]
            out = run(engine, OP_ADD_PRECOMP, raw_rows(pts, neg, 1, q_enc), 1)
            check_coords("p3_add_precomp", out, [to_p3(w) for w in want], [NB] * 4)
            out = run(engine, OP_ADD_PRECOMP, raw_rows(pts, neg | P1P1, 1, q_enc), 1)
            check_coords("p3_add_precomp p1p1", out, want, [NB, AB, NB, NB])
