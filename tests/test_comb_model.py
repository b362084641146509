"""CPU: the comb model of tests/comb_model.py against definitions, and its covering inputs against
both oracles -- so the GPU tests compare only with expectations the reference has already met: every
cover signature and block is accepted by the pure-Python predicate and by the C oracle, every control
is rejected by both, and the covers hold every reachable (row, digit) pair."""
import random

import numpy as np
import pytest

import comb_model as CM
import msm_model as MM
import oracle as O
import zip215 as Z


# ---- recode256 ----
def check_digits(s):
    d = CM.recode256(s)
    assert len(d) == 32 and all(-128 <= x <= 127 for x in d)
    assert CM.from_digits(d) == s
    if s < Z.L:
        assert CM.top_carry(s) == 0 and 0 <= d[31] <= 16
    assert [((w >> (8 * k) & 0xFF) ^ 0x80) - 0x80 for w in CM.packed(d) for k in range(4)] == d
    return d


def test_recode256_edges():
    E = CM.EDGES
    assert all(v < Z.L for v in E.values())
    assert check_digits(E["zero"]) == [0] * 32
    assert check_digits(E["one"]) == [1] + [0] * 31
    check_digits(E["l_minus_1"])
    assert check_digits(E["two_252"]) == [0] * 31 + [16]
    assert E["all_7f"].to_bytes(32, "little") == b"\x7f" * 31 + b"\x0f"
    assert check_digits(E["all_7f"]) == [127] * 31 + [15]
    assert E["all_minus_128"].to_bytes(32, "little") == b"\x80" + b"\x7f" * 30 + b"\x0f"
    assert check_digits(E["all_minus_128"]) == [-128] * 31 + [16]
    assert E["ff_run"].to_bytes(32, "little") == b"\xff" * 31 + b"\x00"
    assert check_digits(E["ff_run"]) == [-1] + [0] * 30 + [1]
    assert E["ff_run_from_80"].to_bytes(32, "little") == b"\x80" + b"\xff" * 30 + b"\x03"
    assert check_digits(E["ff_run_from_80"]) == [-128] + [0] * 30 + [4]
    assert E["top_0f_carry"].to_bytes(32, "little") == bytes(30) + b"\x80\x0f"
    assert check_digits(E["top_0f_carry"]) == [0] * 30 + [-128, 16]
    assert check_digits(E["top_10"])[31] == 16


def test_recode256_random_and_the_top_digit_bound():
    rng = random.Random(5)
    for _ in range(2000):
        check_digits(rng.randrange(Z.L))
    # byte + carry = 128 exactly -> -128; 127 + carry likewise; 255 + carry -> 0 and the carry goes on
    assert CM.recode256(0x80)[:2] == [-128, 1]
    assert CM.recode256(0x7F80)[:3] == [-128, -128, 1]
    assert CM.recode256(0xFF80)[:3] == [-128, 0, 1]
    # no scalar below l reaches 17 in row 31: it needs a top byte of 0x10 and a carry into it
    assert from_17() >= Z.L


def from_17():
    return CM.from_digits([-128] * 31 + [17])  # the smallest scalar whose row-31 digit is 17


# ---- table ----
def test_table_entries_are_the_multiples():
    rng = random.Random(9)
    P = Z.scalarmult(Z.B_POINT, 0x1234567)
    for pt, neg in ((Z.B_POINT, False), (P, True)):
        T = CM.table(pt, neg)
        assert T.shape == (32, 129, 32) and not T[:, :, 27:].any()
        base = Z.neg(pt) if neg else pt
        for i, j in [(0, 0), (0, 1), (0, 128), (1, 1), (31, 128), (31, 16), (17, 77)] + \
                [(rng.randrange(32), rng.randrange(129)) for _ in range(12)]:
            x, y = MM.affine(Z.scalarmult(base, j << (8 * i)))[:2]
            assert CM.entry_values(T[i, j]) == ((y + x) % Z.P, (y - x) % Z.P, 2 * Z.D * x * y % Z.P), (i, j)
            assert all(int(w) < 1 << 29 for w in T[i, j])
    assert CM.entry_values(CM.table(Z.B_POINT)[5, 0]) == (1, 1, 0)  # the identity


def test_table_of_small_order_points_collapses():
    for enc, _ in Z.small_order_encodings():
        T = CM.table(Z.decompress(enc), True)
        ident = T[1, 0]
        assert CM.entry_values(ident) == (1, 1, 0)
        assert (T[1:] == ident).all()  # 256 P = O
        assert (T[0, 8] == ident).all() and (T[0, 128] == ident).all()


# ---- covers ----
def arrs(items, pk):
    n = len(items)
    return (np.tile(np.frombuffer(pk, np.uint8), (n, 1)),
            np.array([np.frombuffer(it.sig, np.uint8) for it in items]),
            np.array([np.frombuffer(it.msg, np.uint8) for it in items]))


def both_oracles(items, pk, sigs=None):
    sigs = [it.sig for it in items] if sigs is None else sigs
    pka, _, msg = arrs(items, pk)
    c = O.verify_batch(pka, np.array([np.frombuffer(s, np.uint8) for s in sigs]), msg)
    z = [Z.verify_status(pk, s, it.msg) for it, s in zip(items, sigs)]
    return [int(x) for x in c], z


def test_b_scalars_recode_as_intended():
    sc = CM.b_scalars()
    assert len(sc) == 258 and len(set(sc)) == 258
    for n, j in enumerate(range(-128, 128)):
        assert CM.recode256(sc[n]) == [j] * 31 + [1 + n % 15]
    assert CM.recode256(sc[256]) == [1] * 31 + [0]
    assert CM.recode256(sc[257]) == [-128] * 31 + [16] and sc[257] >> 248 == 0x0F
    got = CM.pairs_of(CM.b_cover(), "s")
    assert {(i, d) for i in range(31) for d in range(-128, 128)} <= got
    assert {d for i, d in got if i == 31} == set(CM.TOP_DIGITS)
    assert len(got) == CM.PAIRS == 7953


def test_b_cover_verifies_under_every_small_order_key_and_controls_do_not():
    items = CM.b_cover()
    assert [CM.sig_s(it.sig) for it in items] == CM.b_scalars()
    com = CM.committee()
    pk = com.pks[com.small].tobytes()
    c, z = both_oracles(items, pk)
    assert c == z == [0] * len(items)
    for enc, _ in Z.small_order_encodings()[::3]:  # ... and under the other small-order keys
        assert not O.verify_batch(*arrs(items[::17], enc)).any()
    ctl = CM.controls(items)
    assert [i for _, i, _ in ctl] == list(range(32))
    c, z = both_oracles([items[n] for n, _, _ in ctl], pk, [s for _, _, s in ctl])
    assert c == z == [1] * 32


@pytest.mark.parametrize("key", CM.committee().a_keys)
def test_a_cover_is_complete_and_verifies(key):
    com = CM.committee()
    assert com.a_keys == (0, 3, 4) and com.small == 2 and len(com.pks) == 5
    pk = com.pks[key].tobytes()
    assert Z.point_eq(Z.decompress(pk), Z.scalarmult(Z.B_POINT, com.secrets[key]))
    items = CM.key_cover(key)
    assert len(CM.pairs_of(items)) == CM.PAIRS and len(items) < 1000
    for it in items[::50]:
        k = Z.sha512_mod_l(it.sig[:32], pk, it.msg)
        assert list(it.k_digits) == CM.recode256(k) and list(it.s_digits) == CM.recode256(CM.sig_s(it.sig))
    c, z = both_oracles(items, pk)
    assert c == z == [0] * len(items)
    ctl = CM.controls(items)
    c, z = both_oracles([items[n] for n, _, _ in ctl], pk, [s for _, _, s in ctl])
    assert c == z == [1] * 32


def test_sub_cover_holds_its_pairs():
    want = CM.sub_pairs()
    assert len(want) == 8 * 5 + 2  # row 31 holds 0 and 1 of the five digits
    sub = CM.sub_cover(CM.key_cover(0))
    assert want <= CM.pairs_of(sub) and len(sub) <= len(want)
    assert want <= CM.pairs_of(CM.sub_cover(CM.b_cover(), "s"), "s")


def test_block_covers_pass_the_block_oracle_and_controls_fail_on_the_signature():
    com = CM.committee()
    key = com.a_keys[1]
    a_blocks, b_blocks = CM.block_a_cover(key), CM.block_b_cover()
    assert len(CM.pairs_of([b.item for b in a_blocks])) == CM.PAIRS
    assert len(CM.pairs_of([b.item for b in b_blocks], "s")) == CM.PAIRS
    for blocks, author in ((a_blocks, key), (b_blocks, com.small)):
        pk = com.pks[author].tobytes()
        for b in blocks:
            st, md, bd = O.block_verify(b.bincode, com.pks, com.stakes, 0)
            assert (st, md, bd) == (0, b.msg_digest, b.digest)
            assert b.bincode[-64:] == b.item.sig and Z.verify_status(pk, b.item.sig, b.msg_digest) == 0
        for n, i, c in CM.block_controls(blocks):
            st, md, bd = O.block_verify(c.bincode, com.pks, com.stakes, 0)
            assert (st, md, bd) == (6, c.msg_digest, c.digest), (n, i)  # BLOCK_SIG_INVALID, digests still right
            assert Z.verify_status(pk, c.bincode[-64:], c.msg_digest) == 1
