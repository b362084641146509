"""The rule of mv_encode_blocks (include/mysti_verify.h, "encoding blocks") in plain Python over lists
and bytes: statuses, lengths, the padded layout and the cap rule, with a strict statement reader of
its own. No numpy, no library: the GPU, the sanitized host harness and blocks.encode are held to it.

A payload is one bincode::serialize(&Vec<BaseStatement>) string (core.rs:217-224): a u64 count, then
the statements (types.rs:100-114). A block is: own reference (authority, round, 32, 32 zero bytes), k,
k include references, the statement count, the payload bodies, time low, time high, the marker byte,
the epoch, 64, 64 zero bytes."""
import struct
from typing import List, NamedTuple, Optional, Sequence

OK, BAD_HEAD, BAD_PAYLOAD, TOO_LONG = range(4)
STATUS = ["OK", "BAD_HEAD", "BAD_PAYLOAD", "TOO_LONG"]
MAP_SIZE, HEADER_LEN_BYTES = 0x1000000, 16  # wal.rs:96-97, 110
MAX_LEN = (MAP_SIZE - HEADER_LEN_BYTES) // 2  # wal.rs:107 and core.rs:300: MAX_ENTRY_SIZE / 2
HEAD_WORDS = 10
U64 = 2**64 - 1


class Short(Exception):
    pass


class Reader:
    """Fails (Short) when a read runs past the end."""

    def __init__(self, b: bytes):
        self.b, self.pos = b, 0

    def take(self, k: int) -> bytes:
        if k > len(self.b) - self.pos:
            raise Short()
        self.pos += k
        return self.b[self.pos - k:self.pos]

    def u64(self) -> int:
        return struct.unpack("<Q", self.take(8))[0]

    def u32(self) -> int:
        return struct.unpack("<I", self.take(4))[0]

    def ref(self):
        a, r, l = self.u64(), self.u64(), self.u64()
        if l != 32:
            raise Short()
        return a, r, self.take(32)


def read_statement(r: Reader):
    tag = r.u32()
    if tag == 0:
        return ("share", r.take(r.u64()))
    if tag == 1:
        ref, off, vote = r.ref(), r.u64(), r.u32()
        if vote == 0:
            return ("accept", ref, off)
        if vote != 1:
            raise Short()
        some = r.take(1)[0]
        if some == 0:
            return ("reject", ref, off, None)
        if some != 1:
            raise Short()
        return ("reject", ref, off, (r.ref(), r.u64()))
    if tag == 2:
        return ("range", r.ref(), r.u64(), r.u64())
    raise Short()


def read_payload(b: bytes):
    """The statements of a payload, None unless it deserializes and ends on its last byte."""
    r = Reader(b)
    try:
        count = r.u64()
        if count > len(b):  # (every statement has at least 12 bytes: no loop over a count the bytes cannot hold)
            return None
        sts = [read_statement(r) for _ in range(count)]
    except Short:
        return None
    return sts if r.pos == len(b) else None


# ---------------------------------------------------------------- writers (for the tests' inputs)
def ref_bin(ref) -> bytes:
    return struct.pack("<QQQ", ref[0], ref[1], 32) + ref[2]


def statement_bin(st) -> bytes:
    if st[0] == "share":
        return struct.pack("<IQ", 0, len(st[1])) + st[1]
    if st[0] == "accept":
        return struct.pack("<I", 1) + ref_bin(st[1]) + struct.pack("<QI", st[2], 0)
    if st[0] == "reject":
        tail = b"\x00" if st[3] is None else b"\x01" + ref_bin(st[3][0]) + struct.pack("<Q", st[3][1])
        return struct.pack("<I", 1) + ref_bin(st[1]) + struct.pack("<QI", st[2], 1) + tail
    assert st[0] == "range"
    return struct.pack("<I", 2) + ref_bin(st[1]) + struct.pack("<QQ", st[2], st[3])


def payload(statements: Sequence) -> bytes:
    return struct.pack("<Q", len(statements)) + b"".join(statement_bin(s) for s in statements)


def ref_words(ref) -> List[int]:
    """A reference as an include row: authority, round, four little-endian digest words."""
    return [ref[0], ref[1]] + list(struct.unpack("<4Q", ref[2]))


def head(author, rnd, time_ns, epoch, marker, inc0, k, pay0, npay) -> List[int]:
    return [author, rnd, time_ns & U64, time_ns >> 64, epoch, marker, inc0, k, pay0, npay]


# ---------------------------------------------------------------- the rule
class Result(NamedTuple):
    buf: Optional[bytearray]  # None: the total exceeded cap, nothing was written
    offs: List[int]
    lens: List[int]
    status: List[int]
    out_bytes: int


def block_bytes(h, includes, bodies, count) -> bytes:
    inc0, k = h[6], h[7]
    out = [struct.pack("<QQQ", h[0], h[1], 32), bytes(32), struct.pack("<Q", k)]
    for row in includes[inc0:inc0 + k]:
        out.append(struct.pack("<QQQ4Q", row[0], row[1], 32, *row[2:6]))
    out.append(struct.pack("<Q", count))
    out.extend(bodies)
    out.append(struct.pack("<QQBQQ", h[2], h[3], h[5], h[4], 64) + bytes(64))
    return b"".join(out)


def encode(heads, includes, payload_buf: bytes, payload_off, payload_len, cap: Optional[int] = None,
           out: Optional[bytearray] = None) -> Result:
    """heads: rows of 10 integers; includes: rows of 6. cap None: room for everything. `out` (cap =
    its length unless given) is written in place; bytes behind the span keep what they held."""
    m, p = len(includes), len(payload_off)
    checked = {}

    def check(j):
        if j not in checked:
            o, l = payload_off[j], payload_len[j]
            sts = read_payload(payload_buf[o:o + l]) if o + l <= len(payload_buf) else None
            checked[j] = None if sts is None else (len(sts), payload_buf[o + 8:o + l])
        return checked[j]

    blocks, status = [], []
    for h in heads:
        assert len(h) == HEAD_WORDS and all(0 <= w <= U64 for w in h)
        if h[5] > 1 or h[6] + h[7] > m or h[8] + h[9] > p:
            status.append(BAD_HEAD)
            blocks.append(b"")
            continue
        got = [check(j) for j in range(h[8], h[8] + h[9])]
        if any(g is None for g in got):
            status.append(BAD_PAYLOAD)
            blocks.append(b"")
            continue
        length = 169 + 56 * h[7] + sum(len(g[1]) for g in got)
        if length > MAX_LEN:
            status.append(TOO_LONG)
            blocks.append(b"")
            continue
        b = block_bytes(h, includes, [g[1] for g in got], sum(g[0] for g in got))
        assert len(b) == length
        status.append(OK)
        blocks.append(b)
    offs, pos = [], 0
    for b in blocks:
        offs.append(pos)
        pos += (len(b) + 7) & ~7
    lens = [len(b) for b in blocks]
    if cap is None:
        cap = pos if out is None else len(out)
    if pos > cap:
        return Result(None, offs, lens, status, pos)
    if out is None:
        out = bytearray(cap)
    for o, b in zip(offs, blocks):
        out[o:o + ((len(b) + 7) & ~7)] = b + bytes(-len(b) % 8)
    return Result(out, offs, lens, status, pos)
