"""The case lists of mv_encode_blocks that tests/test_encode_model.py, tests/test_encode_sanitized.py
and tests/test_gpu_encode.py share: calls (heads, include rows, a payload buffer and its list) built
from plain Python values. The shapes are the smallest at which the kernels can go wrong: include
counts around the wave width, payload counts around the LDS step and the LDS tile, every statement
kind, every source alignment, blocks either side of the wave / workgroup switch."""
import hashlib
import struct

import encode_model as EM

WG_BYTES = 4096  # kernels.h EN_WG_BYTES: from here on a workgroup writes the block
TILE = 512       # kernels.h EN_TILE: up to here a block's boundaries are kept in LDS


def digest(*key) -> bytes:
    return hashlib.blake2b(repr(key).encode(), digest_size=32).digest()


def ref(a, r):
    return (a, r, digest("ref", a, r))


class Call:
    """One mv_encode_blocks call under construction."""

    def __init__(self, name):
        self.name = name
        self.heads, self.includes = [], []
        self.pbuf, self.poff, self.plen = bytearray(), [], []
        self.want = []  # the status each block is built to get

    def pay(self, b: bytes, align=None) -> int:
        """Appends a payload (at byte offset `align` mod 8 when given): its index in the list."""
        if align is not None:
            self.pbuf += b"\xee" * ((align - len(self.pbuf)) % 8)
        self.poff.append(len(self.pbuf))
        self.plen.append(len(b))
        self.pbuf += b
        return len(self.poff) - 1

    def span(self, off, length) -> int:
        """A payload entry over bytes that are there already (or are not)."""
        self.poff.append(off)
        self.plen.append(length)
        return len(self.poff) - 1

    def block(self, author, rnd, refs, pay0=0, npay=0, time_ns=None, epoch=0, marker=0, want=EM.OK, inc0=None, k=None):
        if inc0 is None:
            inc0 = len(self.includes)
            self.includes += [EM.ref_words(x) for x in refs]
        time_ns = rnd * 10**8 + author if time_ns is None else time_ns
        self.heads.append(EM.head(author, rnd, time_ns, epoch, marker, inc0, len(refs) if k is None else k, pay0, npay))
        self.want.append(want)
        return len(self.heads) - 1

    def model(self, cap=None, out=None):
        return EM.encode(self.heads, self.includes, bytes(self.pbuf), self.poff, self.plen, cap=cap, out=out)

    def without(self, drop):
        """The same call less the blocks in `drop` (inputs otherwise untouched)."""
        c = Call(self.name + " less " + str(sorted(drop)))
        c.heads = [h for i, h in enumerate(self.heads) if i not in drop]
        c.want = [w for i, w in enumerate(self.want) if i not in drop]
        c.includes, c.pbuf, c.poff, c.plen = self.includes, self.pbuf, self.poff, self.plen
        return c


SHARE_SIZES = (0, 1, 7, 8, 9, 127, 128, 129, 512)


def every_kind():
    """One statement of every kind, Shares of every size of SHARE_SIZES."""
    a, b = ref(2, 9), ref(1, 8)
    sts = [("share", bytes((7 * i + n) & 0xff for i in range(n))) for n in SHARE_SIZES]
    sts += [("accept", a, 5), ("reject", a, 6, None), ("reject", b, 7, (a, 3)), ("range", b, 2, 11)]
    return sts


def shapes():
    """Case list 1: everything here is MV_ENCODE_OK."""
    c = Call("shapes")
    prev = [ref(a, 1) for a in range(512)]
    empty = EM.payload([])
    # include counts, no payload
    for k in (0, 1, 63, 64, 65, 67, 100, 512):
        c.block(k % 7, 2, prev[:k])
    # one empty payload; five payloads with empties between them; a non-zero high time word; marker 1
    e = c.pay(empty)
    c.block(1, 2, prev[:3], e, 1)
    first = c.pay(EM.payload([("share", b"abc")]))
    c.pay(empty)
    c.pay(EM.payload(every_kind()))
    c.pay(empty)
    c.pay(EM.payload([("range", prev[4], 0, 3), ("share", b"")]))
    c.block(2, 2, prev[:4], first, 5, time_ns=(0x1122334455667788 << 64) | 0x99aabbccddeeff00, epoch=3, marker=1)
    # one payload shared by two blocks: the runs [first + 1, first + 3) and [first + 2, first + 5)
    c.block(3, 2, prev[:2], first + 1, 2)
    c.block(4, 2, prev[:5], first + 2, 3, marker=0)
    # the same payload at each of the 8 source alignments, one block each and one block over all
    body = EM.payload(every_kind()[:10] + [("share", b"tail-of-the-payload")])
    at = [c.pay(body, align=d) for d in range(8)]
    for d in range(8):
        c.block(d % 4, 3, prev[:1 + d], at[d], 1)
    c.block(0, 3, prev[:2], at[0], 8)
    # 65 payloads in one block (the LDS step), and TILE + 9 (a block that searches the scan's array)
    for count in (65, TILE + 9):
        j0 = len(c.poff)
        for j in range(count):
            c.pay(empty if j % 3 == 1 else EM.payload([("share", bytes([j & 0xff]) * (j % 11))]))
        c.block(1, 4, prev[:2], j0, count)
    # every padding length: the tail at each byte of a word
    for extra in range(8):
        c.block(3, 6, prev[:1], c.pay(EM.payload([("share", b"p" * extra)])), 1)
    # one block just under the wave / workgroup switch, one on it
    for size in (WG_BYTES - 1, WG_BYTES, WG_BYTES + 1):
        share = size - 169 - 56 - 12
        j = c.pay(EM.payload([("share", bytes(i * 13 & 0xff for i in range(share)))]), align=5)
        i = c.block(2, 5, prev[:1], j, 1)
    return c


def refusals():
    """Case list 2: refused blocks, each between two blocks that are OK."""
    c = Call("refusals")
    prev = [ref(a, 1) for a in range(8)]
    good_pay = c.pay(EM.payload([("share", b"good"), ("accept", prev[1], 2)]))

    c.includes = [EM.ref_words(x) for x in prev]  # every block's run is a part of these rows

    def good():
        c.block(len(c.heads) % 4, 2, [], good_pay, 1, inc0=len(c.heads) % 5, k=2)

    def bad(pay0, npay=1, want=EM.BAD_PAYLOAD, **kw):
        good()
        kw.setdefault("inc0", 1)
        kw.setdefault("k", 3)
        c.block(1, 2, [], pay0, npay, want=want, **kw)

    small = EM.payload([("share", b"xy"), ("reject", prev[0], 1, (prev[2], 4)), ("range", prev[3], 1, 2)])
    whole = c.pay(small, align=3)
    for cut in range(len(small)):  # cut at every length from 0 to full - 1
        bad(c.span(c.poff[whole], cut))
    c.pay(small + b"\x00")  # one trailing byte
    bad(len(c.poff) - 1)
    r = EM.ref_bin(prev[0])
    raw = {
        "statement tag 3": struct.pack("<QI", 1, 3) + bytes(80),
        "vote tag 2": struct.pack("<QI", 1, 1) + r + struct.pack("<QI", 0, 2),
        "option byte 2": struct.pack("<QI", 1, 1) + r + struct.pack("<QI", 0, 1) + b"\x02" + r + bytes(8),
        "count above the bytes left": struct.pack("<Q", 3) + EM.statement_bin(("share", b"")) * 2,
        "count 2^63": struct.pack("<Q", 1 << 63) + EM.statement_bin(("share", b"")),
        "share length past the end": struct.pack("<QIQ", 1, 0, 5) + b"abcd",
        "share length 2^64 - 1": struct.pack("<QIQ", 1, 0, EM.U64) + b"abcd",
        "digest length word 31": struct.pack("<QI", 1, 2) + struct.pack("<QQQ", 1, 1, 31) + bytes(32) + bytes(16),
    }
    for name, b in raw.items():
        assert EM.read_payload(b) is None, name
        bad(c.pay(b))
    # a good payload in a run with a refused one
    assert good_pay + 1 == whole and c.plen[whole + 1] == 0
    bad(good_pay, 3)
    # spans that leave the payload buffer (the last payload added ends on the buffer's last byte)
    size = len(c.pbuf)
    for off, length in ((size - 4, 5), (size + 1, 0), (EM.U64, 8), (8, EM.U64), (EM.U64 - 3, 8)):
        bad(c.span(off, length))
    # runs that leave m / p, first + count wrapping past 2^64 included; marker 2
    m, p = len(c.includes), len(c.poff)
    for inc0, k in ((m, 1), (m + 1, 0), (0, m + 1), (EM.U64, 2), (2, EM.U64), (1 << 63, 1 << 63)):
        bad(good_pay, 1, want=EM.BAD_HEAD, inc0=inc0, k=k)
    for pay0, npay in ((p, 1), (p + 1, 0), (0, p + 1), (EM.U64, 2), (2, EM.U64), (1 << 63, 1 << 63)):
        bad(pay0, npay, want=EM.BAD_HEAD)
    bad(good_pay, 1, want=EM.BAD_HEAD, marker=2)
    bad(good_pay, 1, want=EM.BAD_HEAD, marker=EM.U64)
    good()
    return c


def too_long():
    """MV_ENCODE_TOO_LONG one unit either side of the limit: the include count that puts the length
    just over it (its span inside m), and a block of exactly the limit. The include rows are one row
    repeated."""
    c = Call("too long")
    k_fit = (EM.MAX_LEN - 169) // 56
    row = EM.ref_words(ref(3, 1))
    c.includes = [row] * (k_fit + 1)
    fill = EM.MAX_LEN - 169 - 56 * k_fit - 12
    assert 0 <= fill < 56
    j = c.pay(EM.payload([("share", bytes(range(fill)))]), align=1)
    j1 = c.pay(EM.payload([("share", bytes(range(fill + 1)))]), align=6)
    c.block(0, 2, [], j, 1, inc0=0, k=k_fit)                       # exactly MV_ENCODE_MAX_LEN
    c.block(1, 2, [], j1, 1, inc0=0, k=k_fit, want=EM.TOO_LONG)    # one byte over, by its payload
    c.block(2, 2, [], 0, 0, inc0=0, k=k_fit + 1, want=EM.TOO_LONG)  # over by its include count
    c.block(3, 2, [], 0, 0, inc0=0, k=EM.U64 // 56 + 1, want=EM.BAD_HEAD)
    c.block(0, 3, [], j, 1, inc0=1, k=2)
    return c
