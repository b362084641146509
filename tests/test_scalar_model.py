"""CPU: the word-level model of the scalar layer (scalar_model.py) against plain big integers, and
the coverage of the case lists the GPU test runs (test_gpu_scalars.py): each list alone is shown to
reach every path of its function, so thinning one fails here."""
import random

import scalar_model as S

L = S.L
T126, T127 = 1 << 126, 1 << 127


def test_constants():
    assert S.val(S.SC_L) == L == (1 << 252) + 27742317777372353535851937790883648493
    assert S.SC_L[4:7] == [0, 0, 0]  # the three zero words a borrow has to cross
    assert S.val(S.SC_MU) == (1 << 512) // L and S.SC_MU[8] == 0xF
    assert S.QMAX == S.MU  # 2^512 is no multiple of l


# ---- sc_reduce512 ----
def test_reduce_model_and_cases():
    xs = S.reduce_cases()
    assert len(xs) <= 3000 and all(0 <= x < 1 << 512 for x in xs)
    res = {x: S.reduce512(x) for x in xs}
    for x, m in res.items():
        assert m.r == x % L, hex(x)
        assert m.q3 == ((x >> 224) * S.MU) >> 288
        assert m.short == m.corrections and m.short in (0, 1), hex(x)
        assert m.wrapped == (x % (1 << 288) < m.q3 * L % (1 << 288))
        assert m.rr8 == (0, 0, 0)  # x - q3 l < 2 l: word 8 is clear whatever borrowed on the way
    # both branches end in remainder 0 and 1; remainder 0 without a correction is x = 0 alone
    for cor in (0, 1):
        for rem in (0, 1):
            assert any(m.corrections == cor and m.r == rem for m in res.values()), (cor, rem)
    assert [x for x, m in res.items() if m.corrections == 0 and m.r == 0] == [0]
    assert sum(m.corrections == 0 and m.r == L - 1 for m in res.values()) >= 20
    # a remainder of l - 1 is out of the correction's reach: the estimate is short by less than
    # 0.2250 (test_reduce_estimate_is_at_most_one_short), so a corrected x has x mod l < 0.2250 l.
    # The lists hold the edge instead: the largest remainder that takes the correction and its
    # successor, which does not, for the smallest and the largest quotients
    assert all(m.r * 10000 < 2250 * L for m in res.values() if m.corrections)
    for q in (1, (1 << 255), S.QMAX - 1):
        edge = [x - q * L for x, m in res.items() if x // L == q and m.corrections
                and x + 1 in res and not res[x + 1].corrections]
        assert len(edge) == 1 and edge[0] * 10000 < 2250 * L, q
    assert all(m.corrections for x, m in res.items() if x // L == S.QMAX)  # 2^512 - 1 is still inside the reach
    assert max(m.r for m in res.values() if m.corrections) * 10000 > 2249 * L
    # the quotients and offsets
    offs = [0, 1, L - 1, (1 << 224) - 1, 1 << 224]
    for q in (0, 1, 2, S.QMAX - 2, S.QMAX - 1, S.QMAX):
        assert all(q * L + o in res for o in offs if q * L + o < 1 << 512), q
    assert S.QMAX * L + L - 1 >= 1 << 512 > S.QMAX * L + (1 << 224)  # (all that "below 2^512" leaves out)
    sizes = {(x // L).bit_length() for x in xs if x % L == 0}
    assert len(sizes) >= 30 and max(sizes) == 260
    assert sum(m.wrapped for m in res.values()) >= 20
    assert any(m.wrapped and m.corrections == c for m in res.values() for c in (0, 1))
    assert (1 << 512) - 1 in res
    assert all(1 << (32 * i) in res and (1 << (32 * i)) - 1 in res for i in range(16))


def test_reduce_estimate_is_at_most_one_short():
    """The range argument: q3 = floor(floor(x / 2^224) mu / 2^288) with mu = floor(2^512 / l) is
    short of floor(x / l) by  x frac(2^512 / l) / 2^512 + frac(x / 2^224) 2^224 / l  (less a term
    below 2^-288), which is below 0.2249 + 2^-28 < 0.2250 for this l. So the quotient is exact or one
    short, never two: the second conditional subtraction of sc_reduce512 never fires."""
    frac = (1 << 512) % L  # frac(2^512 / l) = frac / l
    assert 2249 * L < 10000 * frac < 2250 * L
    assert (frac << 28) + L < (2250 << 28) * L // 10000  # frac / l + 2^-28 < 0.2250
    r = random.Random(512)
    worst = 0
    for _ in range(100000):
        x = r.randrange(1 << 512)
        short = x // L - (((x >> 224) * S.MU) >> 288)
        assert short in (0, 1), hex(x)
        worst += short
    assert 9000 < worst < 13500  # about 11 % take the one correction
    for x in S.reduce_cases():
        assert S.reduce512(x).short in (0, 1)


# ---- sc_muladd ----
def test_muladd_model_and_cases():
    cs = S.muladd_cases()
    top = (1 << 256) - 1
    assert len(cs) <= 3000
    seen = set()
    for a, b, c in cs:
        assert 0 <= a <= top and 0 <= b <= top and 0 <= c <= top
        m = S.muladd(a, b, c)
        assert m.t == a * b + c and m.r == (a * b + c) % L
        assert m.carry7 == ((a * b) % (1 << 256) + c) >> 256
        seen.add((m.carry7, m.run))
    # no carry, and a carry that runs through 0..7 all-ones words
    assert seen == {(0, 0)} | {(1, j) for j in range(8)}
    for j in range(1, 8):
        m = S.muladd(1 << (32 * j), top, 1 << (32 * j))
        assert (m.carry7, m.run) == (1, j) and m.t == 1 << (256 + 32 * j)
    assert (top, top, top) in cs and (L - 1, L - 1, L - 1) in cs
    assert any(a == 0 for a, b, c in cs) and any(b == 0 for a, b, c in cs) and any(c == 0 and a and b for a, b, c in cs)
    assert any(a < T127 and b == top and c == 0 for a, b, c in cs)        # verify
    assert sum(a < L and b < L and 0 < c < L for a, b, c in cs) >= 20     # sign
    assert sum(a % 8 == 0 and 0 < a < 8 * T127 and b < L and c == 0 for a, b, c in cs) >= 20  # batch


# ---- sc_is_canonical ----
def test_canonical_model_and_cases():
    ss = S.canonical_cases()
    assert len(ss) <= 3000
    for s in ss:
        ok, borrows = S.is_canonical(s)
        assert ok == (s < L), hex(s)
        assert len(borrows) == 8
    for i in range(8):
        assert L + (1 << (32 * i)) in ss and L - (1 << (32 * i)) in ss
        # equal to l above word i, one less in word i where l's word is not zero
        if S.SC_L[i]:
            assert any(s >> (32 * i) == (L >> (32 * i)) - 1 and s % (1 << (32 * i)) == (1 << (32 * i)) - 1 for s in ss), i
    for s in [(1 << 252) + S.L_LOW - 1, (1 << 252) + S.L_LOW + 1, (1 << 252) - 1, (1 << 253) - 1, (1 << 256) - 1]:
        assert s in ss
    assert all(s in ss for s in S.CANONICAL_OLD)
    # a borrow out of word 3 that crosses words 4..6 and is absorbed (or not) by word 7
    crossing = {S.is_canonical(s)[1][3:] for s in ss}
    assert (1, 1, 1, 1, 0) in crossing and (1, 1, 1, 1, 1) in crossing and (0, 0, 0, 0, 0) in crossing
    assert (0, 0, 0, 0, 1) in crossing


# ---- sc_halfsize ----
def _plain_halfsize(k):
    """The remainder sequence on plain integers (no words, no fixed widths)."""
    a, ta, b, tb = L, 0, k, 1
    if b < T126:
        return b, 1
    while True:
        s = a.bit_length() - b.bit_length()
        if (b << s) > a:
            s -= 1
        a -= b << s
        ta -= tb << s
        if a < T126:
            return a, ta
        if a < b:
            a, ta, b, tb = b, tb, a, ta


def test_halfsize_model_and_cases():
    ks, res = S.halfsize_cases(), S.halfsize_results()
    assert len(ks) == len(set(ks)) <= 3000 and all(0 <= k < L for k in ks)
    for k, h in zip(ks, res):
        c, d = _plain_halfsize(k)
        if d < 0:
            c, d = -c, -d
        assert (-h.c if h.c_neg else h.c) == c and h.d == d, hex(k)
        assert (c - d * k) % L == 0 and h.c < T126 and 0 < h.d < T127
        assert max(h.max_ta, h.max_tb) < T127
    have = set(ks)
    for j in range(126, 253):
        assert all((1 << j) + e in have and L - (1 << j) + e in have for e in (-1, 0, 1)), j
    for j in range(1, 127):
        assert L >> j in have and (L >> j) + 1 in have
    assert all(k in have for k in S.HALFSIZE_OLD + S.HALFSIZE_SHORT)
    pairs = set().union(*(h.pairs for h in res))
    assert pairs == S.halfsize_pairs_possible()  # shifts 0..126, both values of `over` from 1 on
    assert {32, 64, 96} <= {s for s, _ in pairs} and {32, 64, 96} <= {s - o for s, o in pairs}
    assert max(h.steps for h in res) >= 170
    assert max(max(h.max_ta, h.max_tb) for h in res) >= T126  # a cofactor with bit 126 set
    assert max(h.d >> 124 for h in res) == 4
    # the longest walk shares its wave with early exits
    longest = max(range(len(res)), key=lambda i: res[i].steps)
    wave = range(longest // 64 * 64, longest // 64 * 64 + 64)
    assert any(ks[i] < T126 and res[i].steps == 0 for i in wave)
    assert sum(res[i].steps >= 120 for i in wave) >= 30


def test_random_halfsize_inputs_stay_on_short_shifts():
    """Why the list is structured: random k never leave the low shifts."""
    r = random.Random(13)
    res = [S.halfsize(r.randrange(L)) for _ in range(2000)]
    assert max(s for h in res for s, _ in h.pairs) < 32
    assert max(h.steps for h in res) < 150


# ---- sc_recode16_128 ----
def test_recode_model_and_cases():
    xs = S.recode_cases()
    assert len(xs) <= 3000
    assert S.RECODE16_128_MAX == 7 * ((1 << 128) - 1) // 15 < T127
    for x in xs:
        assert 0 <= x <= S.RECODE16_128_MAX, hex(x)
        m = S.recode16_128(x)
        assert all(-8 <= d <= 7 for d in m.digits) and m.carry_out == 0
        assert S.from_digits16(m.digits) == x
        assert list(m.words) == S.pack16(m.digits)
        nib = [(x >> (4 * i)) & 15 for i in range(32)]
        assert m.carries[0] == 0 and all(m.carries[i + 1] == (nib[i] + m.carries[i] >= 8) for i in range(31))
    # one past the limit the top nibble overflows, and the digits no longer spell x
    m = S.recode16_128(S.RECODE16_128_MAX + 1)
    assert m.carry_out == 1 and S.from_digits16(m.digits) == S.RECODE16_128_MAX + 1 - (1 << 128)
    have = set(xs)
    assert all(h.c in have and h.d in have for h in S.halfsize_results())
    assert S.RECODE16_128_MAX in have and int("6" + "f" * 30 + "8", 16) in have
    by = {x: S.recode16_128(x) for x in xs}
    assert any(all(d == -8 for d in m.digits[:31]) and m.digits[31] == 7 for m in by.values())
    assert any(all(m.carries[1:]) and m.digits[31] == 7 for m in by.values())  # the carry runs to the top
    assert by[int("6" + "f" * 30 + "8", 16)].digits == (-8,) + (0,) * 30 + (7,)
    assert not any(by[S.RECODE16_128_MAX].carries)
    tops = {(m.digits[31], m.carries[31]) for m in by.values()}
    assert {(t, 0) for t in range(8)} <= tops and {(t, 1) for t in range(1, 8)} <= tops
    assert sum(x < T126 for x in xs) >= 300


# ---- shl_var, len256, the digit readers ----
def test_shl_model_and_cases():
    cs = S.shl_cases()
    assert len(cs) <= 3000
    for x, s in cs:
        assert S.shl_var(x, s, 8) == (x << s) % (1 << 256)
        assert S.shl_var(x % (1 << 128), s, 4) == (x << s) % (1 << 128)
    ones = (1 << 256) - 1
    for s in (0, 1, 31, 32, 33, 63, 64, 95, 96, 127, 128, 255):
        assert (ones, s) in cs and (1, s) in cs
    assert {s for _, s in cs} == set(range(256))
    assert {s >> 5 for x, s in cs if s & 31 == 0 and x == ones} == set(range(8))  # every word shift, no bit shift


def test_len_model_and_cases():
    xs = S.len_cases()
    assert len(xs) <= 3000
    assert all(S.len256(x) == x.bit_length() for x in xs)
    assert 0 in xs and all(1 << n in xs and (1 << (n + 1)) - 1 in xs for n in range(256))


def test_digit_model_and_cases():
    cs = S.digit_cases()
    assert len(cs) <= 3000
    seen256, seen16 = set(), set()
    for sd, kd in cs:
        b = S.val(sd).to_bytes(32, "little")
        d256 = [S.digit256(sd, i) for i in range(32)]
        assert d256 == [x - 256 if x >= 128 else x for x in b]
        d16 = [S.digit16(kd, i) for i in range(64)]
        assert d16 == [((S.val(kd) >> (4 * i)) & 15 ^ 8) - 8 for i in range(64)]
        assert list(sd) == S.pack256(d256) and list(kd) == S.pack16(d16)
        seen256 |= {(i, d) for i, d in enumerate(d256) if all(e == -1 for j, e in enumerate(d256) if j != i)}
        seen16 |= {(i, d) for i, d in enumerate(d16) if all(e == -1 for j, e in enumerate(d16) if j != i)}
    assert seen256 >= {(i, d) for i in range(32) for d in S.DIGIT256_VALUES}
    assert seen16 >= {(i, d) for i in range(64) for d in S.DIGIT16_VALUES}
