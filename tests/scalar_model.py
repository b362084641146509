"""A word-level model of the scalar layer (csrc/scalar25519.h), and the case lists its GPU test
(test_gpu_scalars.py) runs. Nothing here looks at the engine.

Each function works on 32-bit words the way the header does and returns, next to the value, which
path the input took: the Barrett quotient estimate and the number of corrections, the carry run of
sc_muladd's addend, the shifts and the step count of sc_halfsize, the carries of the radix-16
recoding. test_scalar_model.py holds every function to plain big integers and asserts that the case
lists below reach every path, so the lists alone are known to do so.

All lists are deterministic.
"""
import functools
import random
from typing import NamedTuple

import zip215 as Z

L = Z.L
M32 = 0xFFFFFFFF
SC_L = [(L >> (32 * i)) & M32 for i in range(8)]
MU = (1 << 512) // L                      # SC_MU: 9 words
SC_MU = [(MU >> (32 * i)) & M32 for i in range(9)]
L_LOW = L - (1 << 252)                    # l's low 128 bits (125 bits long)
QMAX = ((1 << 512) - 1) // L              # the largest quotient a 512-bit input has


def words(x: int, n: int = 8):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & M32 for i in range(n)]


def val(ws) -> int:
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


# ---- carry32.h ----
def _sub_chain(a, b):
    """a - b word by word (sub_co, subb_co ...): (result words, the borrow out of each word)."""
    out, borrows, bw = [], [], 0
    for x, y in zip(a, b):
        d = x - y - bw
        bw = 1 if d < 0 else 0
        out.append(d & M32)
        borrows.append(bw)
    return out, borrows


def _add_chain(a, b):
    out, carries, c = [], [], 0
    for x, y in zip(a, b):
        s = x + y + c
        c = s >> 32
        out.append(s & M32)
        carries.append(c)
    return out, carries


def _mac_columns(x, y, ncols, ymax=None):
    """Column-wise product as the header's mac loops make it: a 64-bit accumulator whose carry-outs
    are counted in a third word, one output word per column. Pairs (i, k - i) with k - i > ymax are
    left out (the product mod 2^(32 ncols) needs no more)."""
    out, acc, c2 = [], 0, 0
    ymax = len(y) - 1 if ymax is None else ymax
    for k in range(ncols):
        for i in range(len(x)):
            if 0 <= k - i <= ymax:
                acc += x[i] * y[k - i]
                c2 += acc >> 64
                acc &= (1 << 64) - 1
        assert c2 <= M32
        out.append(acc & M32)
        acc = (acc >> 32) | (c2 << 32)
        c2 = 0
    return out, acc


# ---- sc_is_canonical ----
def is_canonical(s: int):
    """(s < l, the borrow out of each of the 8 words of s - l)."""
    _, borrows = _sub_chain(words(s), SC_L)
    return borrows[-1] == 1, tuple(borrows)


# ---- sc_reduce512 ----
class Reduced(NamedTuple):
    r: int            # the 8 result words
    q3: int           # the quotient estimate
    short: int        # floor(x / l) - q3
    corrections: int  # how many of the two conditional subtractions fired
    wrapped: bool     # x mod 2^288 < q3 l mod 2^288: the 9-word subtraction borrowed out
    rr8: tuple        # word 8 of rr after the subtraction and after each conditional step


def reduce512(x: int) -> Reduced:
    xw = words(x, 16)
    q2, top = _mac_columns(xw[7:], SC_MU, 17)
    q2.append(top & M32)
    q3 = q2[9:]
    r2, _ = _mac_columns(q3, SC_L, 9, ymax=7)
    rr, bw = _sub_chain(xw[:9], r2)
    rr8 = [rr[8]]
    corrections = 0
    for _ in range(2):
        s, b2 = _sub_chain(rr, SC_L + [0])
        if b2[-1] == 0:
            rr = s
            corrections += 1
        rr8.append(rr[8])
    return Reduced(val(rr[:8]), val(q3), x // L - val(q3), corrections, bw[-1] == 1, tuple(rr8))


# ---- sc_muladd ----
class MulAdd(NamedTuple):
    r: int
    t: int        # a b + c as the 16 words handed to sc_reduce512
    carry7: int   # the carry of t[0..7] + c out of word 7
    run: int      # how many all-ones words of t[8..15] that carry ran through (0 without a carry)


def muladd(a: int, b: int, c: int) -> MulAdd:
    t, top = _mac_columns(words(a), words(b), 15)
    t.append(top & M32)
    lo, carries = _add_chain(t[:8], words(c))
    cy, run, hi = carries[-1], 0, []
    carry7 = cy
    for w in t[8:]:
        s = w + cy
        if cy and w == M32:
            run += 1
        cy = s >> 32
        hi.append(s & M32)
    assert cy == 0
    tv = val(lo + hi)
    return MulAdd(reduce512(tv).r, tv, carry7, run)


# ---- the recodings and their readers ----
class Recoded(NamedTuple):
    words: tuple     # the 4 packed words
    digits: tuple    # 32 digits in [-8, 7]
    carries: tuple   # the carry into each nibble
    carry_out: int   # the carry that would leave the top nibble: 0 inside the contract


RECODE16_128_MAX = int("7" * 32, 16)  # the largest value 32 digits in [-8, 7] can spell


def recode16_128(x: int) -> Recoded:
    """sc_recode16_128: nibbles from the low end with a carry; nibble + carry >= 8 gives the digit
    nibble + carry - 16 and carry 1. The last carry is dropped, so the digits spell x exactly when
    none leaves the top nibble: x <= RECODE16_128_MAX = 0x7777...7 (every digit 7)."""
    out, digits, carries, carry = [], [], [], 0
    for w in words(x, 4):
        o = 0
        for j in range(8):
            carries.append(carry)
            d = ((w >> (4 * j)) & 15) + carry
            carry = (d + 8) >> 4
            d = (d - (carry << 4)) & 15
            o |= d << (4 * j)
            digits.append((d ^ 8) - 8)
        out.append(o)
    return Recoded(tuple(out), tuple(digits), tuple(carries), carry)


def from_digits16(d) -> int:
    return sum(x << (4 * i) for i, x in enumerate(d))


def pack16(d):
    """Digits in [-8, 7] as 4-bit two's complement, digit i in bits 4 (i % 8).. of word i / 8."""
    out = [0] * ((len(d) + 7) // 8)
    for i, x in enumerate(d):
        out[i >> 3] |= (x & 15) << (4 * (i & 7))
    return out


def pack256(d):
    out = [0] * ((len(d) + 3) // 4)
    for i, x in enumerate(d):
        out[i >> 2] |= (x & 255) << (8 * (i & 3))
    return out


def _sext(v: int, bits: int) -> int:
    return (v ^ (1 << (bits - 1))) - (1 << (bits - 1))


def digit16(kd, i: int) -> int:
    """digit16: the word picked by i / 8, shifted up to the sign bit and arithmetically down."""
    w = kd[i >> 3]
    return _sext(((w << (28 - 4 * (i & 7))) & M32) >> 28, 4)


def digit256(sd, i: int) -> int:
    w = sd[i >> 2]
    return _sext(((w << (24 - 8 * (i & 3))) & M32) >> 24, 8)


# ---- len256, shl_var ----
def len256(x: int) -> int:
    n = 0
    for i, w in enumerate(words(x)):
        if w:
            n = 32 * i + w.bit_length()  # 32 - clz
    return n


def shl_var(x: int, s: int, nw: int) -> int:
    """shl_var<NW>: a funnel shift by s % 32 in every word, then the words moved up by 1, 2 and 4
    as the bits of s / 32 say."""
    assert 0 <= s < 256
    xw = words(x, nw)
    bsh, ws = s & 31, s >> 5
    r = []
    for i in range(nw):
        pair = (xw[i] << 32) | (xw[i - 1] if i else 0)
        r.append((pair >> (32 - bsh)) & M32)
    for k in (1, 2, 4):
        if ws & k:
            r = [r[i - k] if i >= k else 0 for i in range(nw)]
    return val(r)


# ---- sc_halfsize ----
class Half(NamedTuple):
    c: int           # |c|, 4 words
    c_neg: bool
    d: int           # 4 words
    pairs: frozenset  # the (s, over) of every step
    steps: int
    max_ta: int      # the largest cofactor magnitudes met (true integers)
    max_tb: int


M256, M128 = (1 << 256) - 1, (1 << 128) - 1


def halfsize(k: int) -> Half:
    """sc_halfsize on 8-word remainders and 4-word cofactors (two's complement mod 2^128), step for
    step. The true cofactors are carried along: the header's claim that they stay below 2^127 in
    magnitude, which is what lets 4 words hold them, is asserted at every step."""
    assert 0 <= k < L
    a, b, ta, tb = L, k, 0, 1
    Ta, Tb = 0, 1  # the same cofactors as integers
    la, lb = 253, len256(b)
    pairs, steps, max_ta, max_tb = set(), 0, 0, 1
    done = lb <= 126
    if done:
        a, ta, Ta = b, tb, Tb
    while not done:
        s = la - lb
        assert 0 <= s <= 126
        bs = shl_var(b, s, 8)
        x = (a - bs) & M256
        over = 1 if a < bs else 0
        if over:
            assert s >= 1
            x = (x + (bs >> 1)) & M256
        ts = shl_var(tb, s - over, 4)
        ta = (ta - ts) & M128
        Ta -= Tb << (s - over)
        assert abs(Ta) < 1 << 127 and ta == Ta & M128
        pairs.add((s, over))
        steps += 1
        max_ta = max(max_ta, abs(Ta))
        a = x
        la = len256(a)
        if la <= 126:
            done = True
        elif a < b:
            a, b, ta, tb, Ta, Tb, la, lb = b, a, tb, ta, Tb, Ta, lb, la
            max_tb = max(max_tb, abs(Tb))
    c_neg = bool(ta >> 127)
    d = (-ta) & M128 if c_neg else ta
    return Half(a & M128, c_neg, d, frozenset(pairs), steps, max_ta, max_tb)


def halfsize_pairs_possible():
    """Every (s, over) a step can take: s = len(a) - len(b) is 0..126 (len(a) <= 253, len(b) >= 127),
    and b << 0 > a cannot happen, because a >= b holds whenever a step starts."""
    return {(s, o) for s in range(127) for o in (0, 1)} - {(0, 1)}


# ======================================================================= the case lists
def _rand(seed):
    return random.Random(seed)


@functools.lru_cache(maxsize=None)
def reduce_cases():
    """Inputs of sc_reduce512, all below 2^512."""
    r = _rand(113)
    top = (1 << 512) - 1
    xs = [0, top]
    for i in range(17):
        xs += [v for v in ((1 << (32 * i)), (1 << (32 * i)) - 1) if 0 <= v <= top]
    qs = [0, 1, 2, 3, (1 << 31), (1 << 32) - 1, 1 << 32, (1 << 64) - 1, (1 << 96) + 12345, 1 << 128, (1 << 160) - 1,
          (1 << 192) + (1 << 96), 1 << 224, (1 << 252) - 1, L, 1 << 255, (1 << 256) - 1, (1 << 258) + 977,
          QMAX - 2, QMAX - 1, QMAX]
    qs += [r.randrange(1 << n) | 1 << (n - 1) for n in range(8, 260, 12)]
    offs = [0, 1, L - 1, (1 << 224) - 1, 1 << 224]
    for q in qs:
        xs += [q * L + o for o in offs if q * L + o <= top]
    # the edge of the correction: the largest remainder that still needs it, and the next one
    for q in (1, (1 << 128) + 5, 1 << 255, QMAX - 1, QMAX):
        lo, hi = 0, L - 1  # corrections(q l + lo) = 1 (above), corrections(q l + hi) = 0
        if q * L + hi > top:
            hi = top - q * L
        if reduce512(q * L + hi).corrections:  # QMAX: every input with it is corrected
            lo = hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if reduce512(q * L + mid).corrections:
                lo = mid
            else:
                hi = mid
        xs += [q * L + lo, q * L + hi]
    # q l just below a multiple m of 2^288 and x at or just above it: x mod 2^288 is small, q l mod
    # 2^288 is not, and the 9-word subtraction borrows out (m 2^288 - 1 is the same q without it)
    for m in (1, 2, (1 << 100) + 3, (1 << 223) + 1, (1 << 224) - 1):
        q = (m << 288) // L
        xs += [(m << 288) - 1, m << 288, (m << 288) + 1, q * L + L - 1]
    xs += [L * L, 2 * L, L + 1, 1 << 256]
    xs += [r.randrange(1 << 512) for _ in range(300)]
    return tuple(dict.fromkeys(xs))


@functools.lru_cache(maxsize=None)
def muladd_cases():
    """(a, b, c) of sc_muladd, each below 2^256."""
    r = _rand(112)
    top = (1 << 256) - 1
    out = [(top, top, top), (0, top, top), (top, 0, top), (top, top, 0), (0, 0, 0), (0, 0, top), (1, 1, 0)]
    # the carry out of word 7 runs through j all-ones words
    out += [(1 << (32 * j), top, 1 << (32 * j)) for j in range(1, 8)]
    out += [(top, 1 << (32 * j), 1 << (32 * j)) for j in range(1, 8)]
    # verify: d < 2^127 times s, no addend
    out += [((1 << 127) - 1, top, 0), ((1 << 127) - 1, L - 1, 0), (1 << 126, L, 0)]
    out += [(r.randrange(1 << 127), r.randrange(1 << 256), 0) for _ in range(20)]
    # sign: r + k a with all three below l
    out += [(L - 1, L - 1, L - 1), (L - 1, 1, L - 1), (1, L - 1, 1)]
    out += [(r.randrange(L), r.randrange(L), r.randrange(L)) for _ in range(20)]
    # batch: 8 z times k
    out += [(8 * ((1 << 127) - 1), L - 1, 0)]
    out += [(8 * r.randrange(1 << 127), r.randrange(L), 0) for _ in range(20)]
    out += [(r.randrange(1 << 256), r.randrange(1 << 256), r.randrange(1 << 256)) for _ in range(300)]
    return tuple(out)


CANONICAL_OLD = (0, 1, L - 1, L, L + 1, 2**255 - 1, 2**253, 2**252)  # test_gpu_primitives.py's


@functools.lru_cache(maxsize=None)
def canonical_cases():
    """Inputs of sc_is_canonical, below 2^256."""
    r = _rand(114)
    top = (1 << 256) - 1
    ss = list(CANONICAL_OLD)
    for i in range(8):
        ss += [L + (1 << (32 * i)), L - (1 << (32 * i))]
        # word i one below l's (or, where l's word is 0, wrapped to all ones), the words above it
        # l's, the words below it l's, all ones and zero
        hi = L >> (32 * (i + 1)) << (32 * (i + 1))
        wi = ((SC_L[i] - 1) & M32) << (32 * i)
        low_mask = (1 << (32 * i)) - 1
        ss += [hi | wi | (L & low_mask), hi | wi | low_mask, hi | wi]
        # and one above, with nothing below
        ss += [hi | (((SC_L[i] + 1) & M32) << (32 * i))]
    # the borrow of the low 128 bits has to cross l's three zero words
    ss += [(1 << 252) + L_LOW + e for e in (-1, 0, 1)] + [L_LOW - 1, L_LOW, (1 << 128) - 1]
    ss += [(1 << 252) - 1, (1 << 253) - 1, top]
    ss += [r.randrange(1 << 256) for _ in range(100)] + [r.randrange(1 << 253) for _ in range(100)]
    return tuple(dict.fromkeys(s for s in ss if 0 <= s <= top))


def _fib_pair(bits=260):
    a, b = 1, 1
    while b.bit_length() < bits:
        a, b = b, a + b
    return a, b


HALFSIZE_OLD = (0, 1, 2, 2**126 - 1, 2**126, 2**126 + 1, 2**200 + 5, 2**252, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2,
                2**252 - 1, 3 * 2**126, L // 3, L // 5 + 7)  # test_gpu_primitives.py's
HALFSIZE_SHORT = (0, 1, 2**64, 2**125 + 1, 2**126 - 1)  # the early exit: k itself is short


@functools.lru_cache(maxsize=None)
def halfsize_cases():
    """k of sc_halfsize, all below l (sc_halfsize takes k < l: `l >> 0` and its successor are left
    out). The first wave of 64 rows holds the longest-running values next to the early exits."""
    ks = []
    for j in range(126, 253):
        ks += [(1 << j) + e for e in (-1, 0, 1)]
        ks += [L - (1 << j) + e for e in (-1, 0, 1)]
    for j in range(0, 127):
        ks += [L >> j, (L >> j) + 1]
    fn, fn1 = _fib_pair()
    g = L * fn // fn1
    ks += [g, g + 1, L - g]
    ks += list(HALFSIZE_OLD)
    r = _rand(116)
    ks += [r.randrange(L) for _ in range(200)]
    ks = [k for k in dict.fromkeys(ks) if 0 <= k < L and k not in HALFSIZE_SHORT]
    longest = sorted(ks, key=lambda k: -halfsize(k).steps)[:32]
    first = []
    for i, k in enumerate(longest):  # one short k after every few long ones
        first.append(k)
        if i % 6 == 0:
            first.append(HALFSIZE_SHORT[(i // 6) % len(HALFSIZE_SHORT)])
    rest = [k for k in ks if k not in set(longest)]
    return tuple(dict.fromkeys(first + list(HALFSIZE_SHORT) + rest))


@functools.lru_cache(maxsize=None)
def halfsize_results():
    return tuple(halfsize(k) for k in halfsize_cases())


@functools.lru_cache(maxsize=None)
def recode_cases():
    """x of sc_recode16_128, every one inside the contract x <= RECODE16_128_MAX."""
    r = _rand(115)
    xs = []
    for h in halfsize_results():
        xs += [h.c, h.d]
    xs += [
        0, 1, 7, 8,
        from_digits16([-8] * 31 + [7]),   # every digit below the top one -8: nibbles 8, 7, 7, ..., top 6 plus the carry
        int("0" + "8" * 31, 16),          # nibbles all 8 below a top nibble of 0
        int("6" + "8" * 31, 16),          # and below a top nibble of 6, which the carry makes 7
        int("7" * 32, 16),                # nibbles all 7: no carry anywhere, the largest value in the contract
        int("6" + "f" * 30 + "8", 16),    # the carry runs through every nibble into a top nibble of 6
        int("0" + "f" * 30 + "8", 16),
        int("4" + "f" * 31, 16),          # the largest d's top nibble, with the carry in
        (1 << 126) - 1, 1 << 126, (1 << 127) - 1 - int("8" * 31, 16),
    ]
    xs += [t << 124 for t in range(8)] + [t << 124 | 8 << 120 for t in range(7)]  # every top digit, without and with a carry in
    xs += [r.randrange(1 << 126) for _ in range(300)]
    return tuple(dict.fromkeys(xs))


SHIFTS4 = (0, 1, 31, 32, 33, 63, 64, 95, 96, 127)
SHIFTS8 = SHIFTS4 + (128, 129, 159, 160, 161, 191, 192, 223, 224, 225, 254, 255)


@functools.lru_cache(maxsize=None)
def shl_cases():
    """(x, s) of shl_var: x has 8 words (shl_var<4> takes the low four); s < 256."""
    r = _rand(117)
    xs = [(1 << 256) - 1] + [1 << n for n in (0, 1, 31, 32, 63, 64, 96, 127, 128, 159, 160, 255)]
    xs += [r.randrange(1 << 256) for _ in range(6)]
    out = [(x, s) for x in xs for s in SHIFTS8]
    out += [(r.randrange(1 << 256), s) for s in range(256)]  # every shift once
    return tuple(out)


@functools.lru_cache(maxsize=None)
def len_cases():
    r = _rand(118)
    xs = [0] + [1 << n for n in range(256)] + [(1 << n) - 1 for n in range(1, 257)]
    xs += [(1 << n) | 1 for n in (32, 64, 224, 255)] + [r.randrange(1 << r.randrange(1, 257)) for _ in range(60)]
    return tuple(dict.fromkeys(xs))


DIGIT256_VALUES = (-128, -1, 0, 127)
DIGIT16_VALUES = (-8, -1, 0, 7)


@functools.lru_cache(maxsize=None)
def digit_cases():
    """(sd words, kd words): every digit position holding each of the edge values among neighbours
    that are all ones (digit -1), in both packings. Row n places radix-256 value n % 4 at byte
    n / 4 % 32 and radix-16 value n % 4 at nibble n / 4 (n < 256)."""
    r = _rand(119)
    out = []
    for n in range(256):
        d256 = [-1] * 32
        d256[(n // 4) % 32] = DIGIT256_VALUES[n % 4]
        d16 = [-1] * 64
        d16[n // 4] = DIGIT16_VALUES[n % 4]
        out.append((tuple(pack256(d256)), tuple(pack16(d16))))
    for _ in range(40):
        out.append((tuple(words(r.randrange(1 << 256))), tuple(words(r.randrange(1 << 256)))))
    return tuple(out)
