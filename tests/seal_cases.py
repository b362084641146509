"""Helper (not a test): the link-rule corpus shared by the model's CPU test and the GPU test of
mv_seal_blocks -- every case of the rule in include/mysti_verify.h in one linked call."""
import struct

from mysticeti_amd import blocks as BL

N_AUTH = 5
STALE = bytes([0x5A]) * 32  # what an include's digest bytes hold when nothing links them


def seeds():
    return [BL.authority_seed(a) for a in range(N_AUTH)]


def blk(a, r, inc, n_extra=0):
    """An unsealed block (zero digest and signature) of authority a, round r, with a Share of n_extra bytes."""
    return BL.encode(a, r, inc, [b"t" * n_extra] if n_extra else [], [], r * 100 + a, 0, bytes(64), bytes(32))[0]


def overcount(b, count):
    """b with its include count word (byte 56) replaced."""
    b = bytearray(b)
    struct.pack_into("<Q", b, 56, count)
    return bytes(b)


def link_corpus():
    """(blocks, expected status names, {block: expected include digests as indices into bd or STALE})."""
    g = BL.genesis_refs(N_AUTH)
    blocks = [
        blk(0, 1, [g[0]]),                                 # 0
        blk(0, 1, [g[0]], n_extra=5),                      # 1 equivocates with 0: the lowest index holds the key
        blk(1, 1, [g[1], (0, 1, STALE)]),                  # 2 includes a block of its own round: UNLINKED
        blk(2, 1, [g[2], (0, 2, STALE)]),                  # 3 includes a block at a higher index: UNLINKED
        blk(3, 1, [g[3]])[:-1],                            # 4 cut by one byte: parse error; the only block of (3, 1)
        blk(9, 1, [g[0]]),                                 # 5 unknown author
        overcount(blk(4, 1, [g[4]]), 2**40),               # 6 include count past the length: parse error; the only (4, 1)
        blk(0, 2, [(0, 1, STALE), (1, 1, STALE), (2, 1, STALE), (3, 1, STALE), (4, 1, STALE), (9, 1, STALE),
                   (7, 1, STALE)]),                        # 7
        blk(1, 5, [(0, 2, STALE), (1, 2, STALE)]),         # 8 a round gap (1, 2, 5)
    ]
    status = ["OK", "OK", "UNLINKED", "UNLINKED", "PARSE_ERROR", "UNKNOWN_AUTHOR", "PARSE_ERROR", "OK", "OK"]
    # 7: (0, 1) -> block 0, not its equivocation; (1, 1) and (2, 1) were left unlinked: no fresh
    # digest; (3, 1) and (4, 1) are held by parse-error blocks alone, whose authority and round are
    # still readable: a parse error never matches; (9, 1): nor does an unknown author; (7, 1): no
    # such block.  8: (1, 2) is not in the call
    links = {7: [0, STALE, STALE, STALE, STALE, STALE, STALE], 8: [7, STALE]}
    return blocks, status, links
