"""A plain big-integer model of the radix-256 comb tables (csrc/comb.h, k_comb_init) and of the
digits their consumers look up (sc_recode256, scalar25519.h), over oracle/zip215.py's point
arithmetic, and the inputs that reach every table entry through a signature's verdict. Nothing here
looks at the engine.

A table is C[i][j] = [j 256^i](+-P), i = 0..31, j = 0..128, each entry the affine (y+x, y-x, 2dxy)
in canonical 29-bit limbs. A consumer recodes a scalar below l into 32 signed digits d_i in
[-128, 127] and sums C[i][|d_i|] with d_i's sign. A valid signature is accepted only if all of its
64 entries, digits and signs are right, so a set of valid signatures whose digits take every value in
every row turns "accepted" into a check of every reachable entry in the kernel that verified them:

  b_cover()   258 signatures with a chosen s under a small-order key (R = [s]B + T verifies for any
              message): s's digit is j in every row 0..30, j = -128..127, and 0..16 in row 31;
  a_cover()   signatures under a key with a known secret, their messages picked from a stream so
              that the digits of k = SHA-512(R || A || M) mod l take every value in every row.

Reachable: rows 0..30 see every digit -128..127 (entries 0..128, both signs where there are two);
row 31 sees only 0..16, because a scalar below l < 2^252 + 2^125 has a top byte of at most 0x10, and
0x10 plus a carry would need the 31 bytes below it at 0x80.. or more, which is above l - 2^252.
Entries 17..128 of row 31 are built and never read: only the table readback checks them.
"""
import functools
import hashlib
import struct
from typing import NamedTuple, Optional

import numpy as np

import blocks as OB
import msm_model as MM
import zip215 as Z

ROWS, ENTRIES = 32, 129
TOP_DIGITS = range(0, 17)  # what row 31 can hold for a scalar below l
PAIRS = 31 * 256 + len(TOP_DIGITS)  # the reachable (row, digit) pairs: 7,953


# ---- the recoding ----
def recode256(s: int):
    """The 32 signed radix-256 digits of s < 2^253 as sc_recode256 makes them: bytes from the low
    end with a carry; byte + carry >= 128 gives the digit byte + carry - 256 and carry 1. The last
    byte's carry is dropped, as the device's is (none leaves it for s < l)."""
    assert 0 <= s < 1 << 256
    d, carry = [], 0
    for i in range(32):
        x = ((s >> (8 * i)) & 0xFF) + carry
        carry = 1 if x >= 128 else 0
        d.append(x - (carry << 8))
    return d


def top_carry(s: int) -> int:
    """The carry that would leave digit 31."""
    carry = 0
    for i in range(32):
        carry = 1 if ((s >> (8 * i)) & 0xFF) + carry >= 128 else 0
    return carry


def from_digits(d) -> int:
    return sum(x << (8 * i) for i, x in enumerate(d))


def packed(d):
    """The 8 words sc_recode256 writes: digit i as the int8 byte i."""
    raw = bytes(x & 0xFF for x in d)
    return list(struct.unpack("<8I", raw))


# scalars at the recoding's edges (test_comb_model.py shows what each one does)
EDGES = {
    "zero": 0,
    "one": 1,
    "l_minus_1": Z.L - 1,
    "two_252": 1 << 252,
    "all_7f": from_digits([0x7F] * 31 + [0x0F]),          # the largest digits without any carry
    "all_minus_128": from_digits([-128] * 31 + [16]),     # bytes 0x80, 0x7f, ..., top byte 0x0f plus the carry
    "ff_run": from_digits([-1] + [0] * 30 + [1]),          # bytes 0xff x 31: the carry runs through every byte
    "ff_run_from_80": (0x80 | int.from_bytes(b"\xff" * 30, "little") << 8) + (3 << 248),
    "top_0f_carry": from_digits([0] * 30 + [-128, 16]),   # byte 30 = 0x80 alone carries into a top byte of 0x0f
    "top_10": (1 << 252) + 5,                             # a top byte of 0x10 (no carry can reach it below l)
}


# ---- the tables ----
@functools.lru_cache(maxsize=None)
def _table(x: int, y: int) -> np.ndarray:
    base = (x, y, 1, x * y % Z.P)
    pts = []
    for _ in range(ROWS):
        acc = Z.IDENTITY
        pts.append(acc)
        for _ in range(ENTRIES - 1):
            acc = Z.add(acc, base)
            pts.append(acc)
        base = Z.double(acc)  # [256]base = 2 [128]base
    out = np.array([MM.point_row(p) for p in MM.affine_many(pts)], dtype=np.uint32)
    out = out.reshape(ROWS, ENTRIES, 32)
    out.setflags(write=False)
    return out


def table(P, negate: bool = False) -> np.ndarray:
    """(32, 129, 32) uint32: C[i][j] = [j 256^i](+-P) as the device lays an entry out (words 0..8
    y+x, 9..17 y-x, 18..26 2dxy, canonical 29-bit limbs; 27..31 zero). Running additions, one
    doubling per row, one shared inversion. Kept between calls, read-only."""
    x, y = MM.affine(Z.neg(P) if negate else P)[:2]
    return _table(x, y)


def entry_values(row32):
    """(y+x, y-x, 2dxy) mod p of one 32-word entry."""
    w = [int(v) for v in row32]
    return tuple(sum(w[9 * k + i] << (29 * i) for i in range(9)) for k in range(3))


# ---- signatures ----
class Signed(NamedTuple):
    msg: bytes
    sig: bytes
    s_digits: tuple            # the digits of s (the B table's)
    k_digits: Optional[tuple]  # the digits of k (the A table's); None where [k]A is torsion for any k
    cand: int                  # which candidate of the message stream (a_cover), else the cover's index


def sig_s(sig: bytes) -> int:
    return int.from_bytes(sig[32:], "little")


def control(sig: bytes, row: int) -> bytes:
    """The same signature with s + 256^row mod l: [256^row]B is left over, so it must be rejected."""
    return sig[:32] + ((sig_s(sig) + (1 << (8 * row))) % Z.L).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def _mul_b(s: int):
    return Z.scalarmult(Z.B_POINT, s)


def torsion():
    return [p for _, p in sorted(Z.torsion_points().items())]


def b_scalars():
    """The 258 scalars: digit j in every row 0..30 and t_j = 1..15 (cycling) in row 31, j = -128..127;
    then row 31 = 0 (below digits of 1) and row 31 = 16 (below digits of -128: a top byte of 0x0f
    with the carry in). All are in (0, 2^252)."""
    out = []
    for n, j in enumerate(range(-128, 128)):
        out.append(from_digits([j] * 31 + [1 + n % 15]))
    out.append(from_digits([1] * 31 + [0]))
    out.append(from_digits([-128] * 31 + [16]))
    assert all(0 < s < 1 << 252 for s in out)
    return out


@functools.lru_cache(maxsize=None)
def b_cover():
    """A valid signature for each of b_scalars() under any small-order key A: R = [s]B + T, T cycling
    through the eight torsion points, so [8](R - [s]B + [k]A) = [8](T + [k]A) = O whatever the message
    and k. The messages are fixed bytes; a caller may pair the signatures with any others."""
    tors = torsion()
    out = []
    for n, s in enumerate(b_scalars()):
        R = Z.compress(Z.add(_mul_b(s), tors[n % 8]))
        msg = hashlib.sha256(b"comb b cover" + struct.pack("<I", n)).digest()
        out.append(Signed(msg, R + s.to_bytes(32, "little"), tuple(recode256(s)), None, n))
    return tuple(out)


def default_messages(seed: bytes):
    return lambda c: hashlib.sha256(b"comb a cover" + seed + struct.pack("<Q", c)).digest()


def a_cover(a: int, pk: bytes, seed: bytes, message_source=None, candidates: int = 6000, nonces: int = 4):
    """Valid signatures under the key pk = [a]B whose k digits cover every reachable pair: (row i,
    digit d) for i = 0..30, d = -128..127, and (31, d) for d = 0..16 -- all 7,953; the entries left
    out are 17..128 of row 31, which no scalar below l reaches. Asserts the coverage is complete.

    A few nonces r (R = [r]B once each; ZIP-215 does not care how r was derived), messages
    message_source(c) for c = 0, 1, ... (32 bytes each; default: a hash of seed and c), k =
    SHA-512(R || pk || M) mod l. One pass keeps a candidate that holds a pair not yet seen, a second
    drops those whose pairs are all held by others; then s = r + k a mod l. Returns Signed rows,
    cand = c."""
    message_source = message_source or default_messages(seed)
    rs = [Z.sha512_mod_l(b"comb nonce", seed, bytes([n])) for n in range(nonces)]
    Rs = [Z.compress(_mul_b(r)) for r in rs]
    count = {}
    kept = []
    for c in range(candidates):
        msg = message_source(c)
        k = Z.sha512_mod_l(Rs[c % nonces], pk, msg)
        pairs = list(enumerate(recode256(k)))
        if any(p not in count for p in pairs):
            for p in pairs:
                count[p] = count.get(p, 0) + 1
            kept.append((c, msg, k, pairs))
    want = {(i, d) for i in range(31) for d in range(-128, 128)} | {(31, d) for d in TOP_DIGITS}
    assert set(count) == want, f"a_cover: {len(want - set(count))} pairs not covered, {len(set(count) - want)} unexpected"
    out = []
    for c, msg, k, pairs in reversed(kept):  # the late ones were kept for few pairs: try them first
        if all(count[p] > 1 for p in pairs):
            for p in pairs:
                count[p] -= 1
            continue
        s = (rs[c % nonces] + k * a) % Z.L
        out.append(Signed(msg, Rs[c % nonces] + s.to_bytes(32, "little"), tuple(recode256(s)),
                          tuple(d for _, d in pairs), c))
    out.reverse()
    return tuple(out)


def pairs_of(items, which="k"):
    """The (row, digit) pairs a list of Signed holds in its k digits (or its s digits)."""
    got = set()
    for it in items:
        got.update(enumerate(it.k_digits if which == "k" else it.s_digits))
    return got


def controls(items, rows=range(ROWS)):
    """One control per row: (index into items, row, the signature with s + 256^row mod l)."""
    out = []
    for i in rows:
        n = (7 * i + 3) % len(items)
        sig = control(items[n].sig, i)
        assert sig_s(sig) < Z.L and sig != items[n].sig
        out.append((n, i, sig))
    return out


# the sub-cover for one-block-per-call legs: the first and last row of every wave's or role's row
# block (0..15 / 16..31, blocks of 8, blocks of 4 contain them or are met by the full covers), and
# the digits at the ends of the range and around zero
SUB_ROWS = (0, 7, 8, 15, 16, 23, 24, 30, 31)
SUB_DIGITS = (-128, -1, 0, 1, 127)


def sub_pairs():
    return {(i, d) for i in SUB_ROWS for d in SUB_DIGITS if i < 31 or d in TOP_DIGITS}


def sub_cover(items, which="k"):
    """A subset of items (in order) that still holds every pair of sub_pairs() that items holds."""
    need = sub_pairs() & pairs_of(items, which)
    out = []
    for it in items:
        mine = set(enumerate(it.k_digits if which == "k" else it.s_digits)) & need
        if mine:
            need -= mine
            out.append(it)
    assert not need
    return out


# ---- the committee the cover tests share, and whole blocks ----
class Committee(NamedTuple):
    pks: np.ndarray      # (n, 32) uint8
    stakes: np.ndarray   # (n,) uint64
    secrets: tuple       # a with pk = [a]B, or None
    small: int           # the index of the small-order key
    a_keys: tuple        # the indices the A covers are made for: the first, one in between, the last


@functools.lru_cache(maxsize=None)
def committee():
    """Five keys of stake 100: four with known secrets and, at index 2, a point of order 8."""
    secrets, pks = [], []
    t8 = Z.compress(MM.T8)
    for b in range(5):
        if b == 2:
            secrets.append(None)
            pks.append(t8)
        else:
            a = Z.sha512_mod_l(b"comb committee", bytes([b]))
            secrets.append(a)
            pks.append(Z.compress(_mul_b(a)))
    arr = np.frombuffer(b"".join(pks), dtype=np.uint8).reshape(5, 32)
    return Committee(arr, np.full(5, 100, dtype=np.uint64), tuple(secrets), 2, (0, 3, 4))


@functools.lru_cache(maxsize=None)
def key_cover(key: int):
    com = committee()
    return a_cover(com.secrets[key], com.pks[key].tobytes(), bytes([key]))


def _includes():
    # round-1 references of authorities 0..3 (stake 400 of 500: past the threshold clock's quorum);
    # a reference's digest is not checked against a block
    return [OB.BlockReference(a, 1, hashlib.sha256(b"comb include" + bytes([a])).digest()) for a in range(4)]


def block_template(author: int, cand: int):
    """The round-2 block of `author` that candidate `cand` names: only its creation time varies."""
    return OB.StatementBlock(author, 2, _includes(), [("share", b"comb cover")], 2 * 10**8 + cand, False, 0)


def block_messages(author: int):
    """message_source for a_cover: the signed message of block_template(author, c)."""
    return lambda c: block_template(author, c).signed_message()


class Block(NamedTuple):
    bincode: bytes
    msg_digest: bytes
    digest: bytes
    item: Signed


def make_block(author: int, cand: int, sig: bytes, item: Signed) -> Block:
    b = block_template(author, cand)
    b.signature = sig
    b.digest = b.compute_digest()
    return Block(b.bincode(), b.signed_message(), b.digest, item)


@functools.lru_cache(maxsize=None)
def block_a_cover(key: int):
    """a_cover ground over whole blocks of author `key`: (Block, ...)."""
    com = committee()
    items = a_cover(com.secrets[key], com.pks[key].tobytes(), b"blk" + bytes([key]), block_messages(key))
    return tuple(make_block(key, it.cand, it.sig, it) for it in items)


@functools.lru_cache(maxsize=None)
def block_b_cover():
    """b_cover as blocks of the small-order author (the signature verifies for any message)."""
    com = committee()
    return tuple(make_block(com.small, it.cand, it.sig, it) for it in b_cover())


def block_controls(blocks, rows=range(ROWS)):
    """(index, row, Block) per row: the block with its signature's s moved by 256^row (and its digest
    recomputed, so only the signature check fails)."""
    out = []
    for n, i, sig in controls([b.item for b in blocks], rows):
        it = blocks[n].item
        author = int(struct.unpack_from("<Q", blocks[n].bincode, 0)[0])
        out.append((n, i, make_block(author, it.cand, sig, it)))
    return out
