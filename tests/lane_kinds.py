"""Helper (not a test): blocks just over the device ingest's 10 KB LDS window, so that they take the
one-lane walk over global memory (bincode_walk.h under ingest_lane), whose tail is each statement
kind in turn -- Vote Accept, Reject(None), Reject(Some), VoteRange, or nothing after the Share -- and
five blocks malformed at bincode level in the places only that walk's Vote branches read. Built with
oracle/blocks.py and signed by the C oracle; nothing is read from the library."""
import functools
import struct

import numpy as np

import blocks as B
import oracle as O

N_AUTH = 7
STAKES = [3, 1, 1, 2, 1, 1, 1]
SHARE = 10300  # payload bytes: the bincode is past the 10240-byte window at any start alignment
TAILS = ("accept", "reject", "reject_some", "range", "none")
MALFORMED = ("vote tag 2", "option byte 2", "statement tag 3", "cut inside the second locator",
             "second locator's digest length 31")
META = 25 + 8 + 64  # creation time, epoch marker, epoch; the signature's length word and bytes


def committee():
    pks = np.frombuffer(b"".join(O.public_key(B.authority_seed(a)) for a in range(N_AUTH)), dtype=np.uint8)
    return pks.reshape(-1, 32), np.array(STAKES, dtype=np.uint64), 0


def _tail(gen, kind):
    loc, other = B.Locator(gen[3].reference(), 7), B.Locator(gen[5].reference(), 2**40 + 9)
    return {"none": [], "accept": [("accept", loc)], "reject": [("reject", loc, None)],
            "reject_some": [("reject", loc, other)], "range": [("range", gen[4].reference(), 3, 11)]}[kind]


@functools.lru_cache(maxsize=None)
def corpus():
    """([bincode], [name]): 11 well-formed blocks (each tail at two Share lengths, one more without a
    tail), then the five of MALFORMED."""
    gen = [B.genesis(a) for a in range(N_AUTH)]
    rng = np.random.default_rng(1030)

    def block(i, kind, extra):
        a = i % N_AUTH
        inc = [gen[a].reference()] + [gen[x].reference() for x in range(N_AUTH) if x != a]
        sts = [("share", rng.integers(0, 256, size=SHARE + extra, dtype=np.uint8).tobytes())] + _tail(gen, kind)
        return B.new_with_signer(a, 1, inc, sts, 1000 + i, bool(i & 1), 0, B.authority_seed(a), O.sign).bincode()

    bins = [block(i, TAILS[i % 5], 13 * i) for i in range(11)]
    names = [f"tail={TAILS[i % 5]} share={SHARE + 13 * i}" for i in range(11)]

    def patched(kind, at, fmt, value):
        b = bytearray(block(len(bins), kind, 5))
        start = len(b) - META - len(B.statement_bincode(_tail(gen, kind)[0]))  # the tail statement's tag
        struct.pack_into(fmt, b, start + at, value)
        return bytes(b)

    # a Vote: u32 tag, locator (64 bytes), u32 vote, [u8 option, [second locator: authority, round,
    # digest length, digest, offset]]
    some = patched("reject_some", 0, "<I", 1)  # (the tag as it is)
    start = len(some) - META - len(B.statement_bincode(_tail(gen, "reject_some")[0]))
    bins += [patched("accept", 68, "<I", 2), patched("reject", 72, "<B", 2), patched("range", 0, "<I", 3),
             some[:start + 73 + 30], patched("reject_some", 73 + 16, "<Q", 31)]
    names += list(MALFORMED)
    return bins, names


@functools.lru_cache(maxsize=None)
def oracle_results():
    """[(status, message digest, block digest)] of the C oracle, computed once."""
    pks, stakes, epoch = committee()
    return [O.block_verify(b, pks, stakes, epoch) for b in corpus()[0]]
