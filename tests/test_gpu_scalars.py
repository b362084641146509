"""GPU: the functions of csrc/scalar25519.h, each called directly (selftest ops 112..119,
kernels.hip k_selftest_scalar), bit for bit against plain big integers and, where an output
depends on the path taken, against the word-level model (scalar_model.py). The case lists are the
model's; test_scalar_model.py shows on the CPU that they reach every path: both Barrett branches
and the borrow out of 2^288, every carry run of sc_muladd's addend, every shift of sc_halfsize with
both values of `over`, walks of 181 steps next to early exits in one wave, cofactors of 127 bits,
and every carry pattern of the radix-16 recoding.

Every test is one launch over at most a few thousand rows (the digit test: two)."""
import numpy as np
import pytest

import scalar_model as S

pytestmark = pytest.mark.gpu
L = S.L
OP_MULADD, OP_REDUCE, OP_CANONICAL, OP_RECODE16_128, OP_HALFSIZE, OP_SHL, OP_LEN, OP_DIGITS = range(112, 120)
PARAM = 36  # the parameter word of a row


def rows(items, param=None):
    """64-word rows: `items` are lists of words (placed from word 0), `param` the parameter words."""
    w = np.zeros((len(items), 64), dtype=np.uint32)
    for i, it in enumerate(items):
        w[i, :len(it)] = it
    if param is not None:
        w[:, PARAM] = param
    return w


def ints(out, lo, hi):
    """Words lo..hi-1 of every row as one integer each."""
    return [S.val(o[lo:hi]) for o in out]


def test_muladd(engine):
    """sc_muladd(a, b, c) = a b + c mod l for a, b, c < 2^256: the contract's corners, the carry of
    the addend out of word 7 through 0..7 all-ones words, and the shapes verify (d s, no addend),
    signing (r + k a, all below l) and the batch path (8 z times k) call it with."""
    cases = S.muladd_cases()
    out = engine.selftest(OP_MULADD, rows([S.words(a) + S.words(b) + S.words(c) for a, b, c in cases]))
    for (a, b, c), got, o in zip(cases, ints(out, 0, 8), out):
        m = S.muladd(a, b, c)
        assert got == (a * b + c) % L == m.r, (hex(a), hex(b), hex(c), m.carry7, m.run)
        assert not o[8:].any()


def test_reduce512(engine):
    """sc_reduce512(x) = x mod l for x < 2^512: remainders 0, 1 and l - 1 behind quotients of every
    size, with and without the correction; the last remainder that takes the correction and the
    first that does not; inputs whose 9-word subtraction borrows out; 2^512 - 1; every 2^(32 i)
    and 2^(32 i) - 1."""
    cases = S.reduce_cases()
    out = engine.selftest(OP_REDUCE, rows([S.words(x, 16) for x in cases]))
    for x, got, o in zip(cases, ints(out, 0, 8), out):
        m = S.reduce512(x)
        assert got == x % L == m.r, (hex(x), m.corrections, m.wrapped)
        assert not o[8:].any()


def test_is_canonical(engine):
    """sc_is_canonical(s) = (s < l): l +- 2^(32 i), l with one word lowered below equal higher words,
    and the values whose borrow has to cross l's three zero words."""
    cases = S.canonical_cases()
    out = engine.selftest(OP_CANONICAL, rows([S.words(s) for s in cases]))
    for s, o in zip(cases, out):
        assert int(o[0]) == (1 if s < L else 0) == int(S.is_canonical(s)[0]), hex(s)
        assert not o[1:].any()


def test_halfsize(engine):
    """sc_halfsize(k) for k < l: equal to the model, c = d k (mod l), |c| < 2^126 and 0 < d < 2^127.
    The list walks every shift 0..126 with both values of `over`, takes up to 181 steps beside
    lanes that exit at once, and drives the cofactors to 127 bits."""
    cases, want = S.halfsize_cases(), S.halfsize_results()
    out = engine.selftest(OP_HALFSIZE, rows([S.words(k) for k in cases]))
    for k, m, o in zip(cases, want, out):
        c, neg, d = S.val(o[0:4]), int(o[4]), S.val(o[8:12])
        assert (c, neg, d) == (m.c, int(m.c_neg), m.d), (hex(k), m.steps)
        assert ((-c if neg else c) - d * k) % L == 0, hex(k)
        assert c < 1 << 126 and 0 < d < 1 << 127, hex(k)
        assert not o[5:8].any() and not o[12:].any()


def test_recode16_128(engine):
    """sc_recode16_128(x): 32 signed digits in [-8, 7] that spell x. Its contract is that no carry
    leaves the top nibble, which is exactly x <= 0x7777...7 = 7 (2^128 - 1) / 15 (32 nibbles of 7, the
    largest value such digits can spell; the header's sufficient form is x < 2^127 with a top nibble
    of at most 6). Every case is inside it: every c and d of the halfsize list (d's top nibble
    reaches 4), digits all -8 below the top one, nibbles all 7, 0x6ff...f8 whose carry runs through
    every nibble into a top nibble of 6, the limit itself, and random values below 2^126."""
    cases = S.recode_cases()
    assert all(0 <= x <= S.RECODE16_128_MAX for x in cases)
    out = engine.selftest(OP_RECODE16_128, rows([S.words(x, 4) for x in cases]))
    for x, o in zip(cases, out):
        m = S.recode16_128(x)
        got = [((int(w) >> (4 * j) & 15) ^ 8) - 8 for w in o[:4] for j in range(8)]
        assert got == list(m.digits), hex(x)
        assert sum(d << (4 * i) for i, d in enumerate(got)) == x, hex(x)
        assert not o[4:].any()


def test_shl_var(engine):
    """shl_var<8>(x, s) and shl_var<4>(x, s) = x << s mod 2^(32 NW): every s in 0..255, bit shifts of 0,
    1 and 31 under every word shift, on all-ones, single-bit and random words."""
    cases = S.shl_cases()
    out = engine.selftest(OP_SHL, rows([S.words(x) for x, _ in cases], param=[s for _, s in cases]))
    for (x, s), o in zip(cases, out):
        assert S.val(o[0:8]) == (x << s) % (1 << 256) == S.shl_var(x, s, 8), (hex(x), s)
        assert S.val(o[8:12]) == (x << s) % (1 << 128) == S.shl_var(x % (1 << 128), s, 4), (hex(x), s)
        assert not o[12:].any()


def test_len256(engine):
    """len256(x) = the bit length of x: 0, every single bit, every 2^n - 1."""
    cases = S.len_cases()
    out = engine.selftest(OP_LEN, rows([S.words(x) for x in cases]))
    for x, o in zip(cases, out):
        assert int(o[0]) == x.bit_length() == S.len256(x), hex(x)
        assert not o[1:].any()


def test_digit_readers(engine):
    """digit256(sd, i), i = 0..31, and digit16(kd, i), i = 0..63 (through pick8, the index a run-time
    value): every position holding -128, -1, 0, 127 (-8, -1, 0, 7) among neighbours of all ones."""
    cases = S.digit_cases()
    w = [list(sd) + list(kd) for sd, kd in cases]
    out256 = engine.selftest(OP_DIGITS, rows(w, param=0)).astype(np.int32)
    out16 = engine.selftest(OP_DIGITS, rows(w, param=1)).astype(np.int32)
    for n, (sd, kd) in enumerate(cases):
        assert out256[n, :32].tolist() == [S.digit256(sd, i) for i in range(32)], n
        assert not out256[n, 32:].any()
        assert out16[n].tolist() == [S.digit16(kd, i) for i in range(64)], n
