"""Helper (not a test): what tests/test_walk_sanitized.py and tests/test_gpu_span_independence.py share
-- a strict bincode reader of a block, the block of every statement kind and the count attacks on it.
Built with oracle/blocks.py and signed by the C oracle; nothing is read from the library."""
import struct

import numpy as np

import blocks as B
import oracle as O

U64 = (1 << 64) - 1


# ---------------------------------------------------------------- a strict bincode reader of a block's statements
class Short(Exception):
    pass


class Reader:
    def __init__(self, b):
        self.b, self.p = b, 0

    def take(self, n):
        if n > len(self.b) - self.p:
            raise Short()
        at = self.p
        self.p += n
        return at

    def u8(self):
        return self.b[self.take(1)]

    def u32(self):
        return struct.unpack_from("<I", self.b, self.take(4))[0]

    def u64(self):
        return struct.unpack_from("<Q", self.b, self.take(8))[0]

    def ref(self):
        a, r, dl = self.u64(), self.u64(), self.u64()
        if dl != 32:
            raise Short()
        at = self.take(32)
        return (a, r, self.b[at:at + 32])


def decode_block(b):
    """(own reference, statements in votes_cases' form, where the signature ends) of
    bincode(Data<StatementBlock>), or None where bincode fails (types.rs:93-114; trailing bytes allowed,
    data.rs:43-52)."""
    r = Reader(b)
    try:
        own = r.ref()
        for _ in range(r.u64()):
            r.ref()
        sts = []
        for _ in range(r.u64()):
            tag = r.u32()
            if tag == 0:
                ln = r.u64()
                at = r.take(ln)
                sts.append(("share", b[at:at + ln]))
            elif tag == 1:
                ref, off, vote = r.ref(), r.u64(), r.u32()
                if vote == 0:
                    sts.append(("vote", ref, off))
                elif vote == 1:
                    some = r.u8()
                    if some > 1:
                        return None
                    sts.append(("reject", ref, off, (r.ref(), r.u64()) if some else None))
                else:
                    return None
            elif tag == 2:
                sts.append(("range", r.ref(), r.u64(), r.u64()))
            else:
                return None
        r.take(16)
        if r.u8() > 1:
            return None
        r.u64()
        if r.u64() != 64:
            return None
        r.take(64)
        return own, sts, r.p
    except Short:
        return None


def small_committee():
    pks = np.frombuffer(b"".join(O.public_key(B.authority_seed(a)) for a in range(7)), dtype=np.uint8).reshape(-1, 32)
    return pks, np.array([3, 1, 1, 2, 1, 1, 1], dtype=np.uint64), 0


def every_kind_block(share=5):
    """5 includes (a quorum of the small committee), a Share, Vote Accept, Reject(None), Reject(Some)
    and 3 VoteRanges: every statement kind, in config 4's shape."""
    seeds = [B.authority_seed(a) for a in range(7)]
    prev = [B.genesis(a) for a in range(7)]
    inc = [prev[2].reference()] + [prev[x].reference() for x in (0, 1, 3, 4)]
    loc = B.Locator(prev[3].reference(), 4)
    sts = [("share", bytes(k & 0xFF for k in range(share))), ("accept", loc), ("reject", loc, None), ("reject", loc, loc)]
    sts += [("range", prev[4 + k].reference(), k, k + 3) for k in range(3)]
    return B.new_with_signer(2, 1, inc, sts, 1, False, 0, seeds[2], O.sign).bincode(), len(inc)


def count_attacks():
    """[(name, bytes)]: on a valid block, each count or length word in turn set to 2^64 - 1, 2^63,
    2^32, room / size + 1 and room / size (room: the bytes after the word, size: the least bytes of
    what it counts); with size 1 the last two are a Share that reaches one byte past the block's end,
    and exactly its end."""
    blk, n_inc = every_kind_block(40)
    st0 = 64 + 56 * n_inc + 8  # the first statement: a Share's u32 tag, then its length word
    words = {"n_inc": (56, 56), "n_st": (64 + 56 * n_inc, 12), "share length": (st0 + 4, 1), "own digest length": (16, 1),
             "include digest length": (64 + 16, 1), "vote locator digest length": (st0 + 12 + 40 + 4 + 16, 1),
             "signature length": (len(blk) - 72, 1)}
    assert struct.unpack_from("<Q", blk, words["share length"][0])[0] == 40
    assert struct.unpack_from("<Q", blk, words["vote locator digest length"][0])[0] == 32
    out = [("valid", blk)]
    for name, (at, size) in words.items():
        room = len(blk) - at - 8
        for v in (U64, 1 << 63, 1 << 32, room // size + 1, room // size):
            out.append((f"{name} = {v}", blk[:at] + struct.pack("<Q", v) + blk[at + 8:]))
    return out
