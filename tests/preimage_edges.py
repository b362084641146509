"""Helper (not a test): signed blocks whose pre-image P ends, and whose pieces fall, on every edge of
the two Blake2b-256 digests that StatementBlock::verify needs -- B2(P), the signed message, and
B2(P || sig), the block digest (crypto.rs:85-128, types.rs:155-218) -- and on the edges of the
device ingest's LDS window.

  P                    16 (author, round) + 48 per include + the statements + 25 (creation time u128,
                       epoch marker, epoch); a Share is 1 + payload bytes, a Vote 57 (Reject(Some) a
                       second locator of 56 more), a VoteRange 65 (types.rs:661-691, 751-755); the
                       signature's 64 bytes follow in the block digest's input
  edges                |P| % 128 == 0 (P's last block is a full one, the signature starts a fresh
                       one); == 64 (P || sig ends on a boundary); 65..127 (the signature straddles: one
                       block more than B2(P)); every piece kind straddling, ending on and starting on a
                       128-byte boundary; a bincode length at the window's fit test, at every start
                       alignment mod 8

Every size here is len() of what oracle/blocks.py encodes; nothing is read from the library. The
blocks are built with oracle/blocks.py and signed by the C oracle. corpus() is deterministic:
tests/golden/preimage_edges.json pins it."""
import functools
import hashlib

import numpy as np

import blocks as B
import oracle as O

OK, PARSE_ERROR, DIGEST_MISMATCH, GENESIS, SIG_INVALID = O.BLOCK_OK, O.BLOCK_PARSE_ERROR, O.BLOCK_DIGEST_MISMATCH, \
    O.BLOCK_GENESIS, O.BLOCK_SIG_INVALID
N_AUTH = 10
STAKES = [30] + [1] * 9  # total 39, quorum above 2 * 39 // 3 = 26: an include of authority 0 alone passes the clock
EPOCH = 0
TAILS = ("none", "accept", "reject", "reject_some", "range")
RESIDUES = (0, 1, 63, 64, 65, 127)  # |P| % 128 where a schedule changes
TAMPER_RESIDUES = RESIDUES + (128 - 25 + 1,)  # ... and the metadata piece starting one byte before it straddles
WINDOW = 10240  # the device ingest's LDS window (bytes); the fit test is (off & 7) + L + 16 > WINDOW
FIT_VALUES = (WINDOW - 1, WINDOW, WINDOW + 1)
TWO_SHARES_TOTAL = 200
FAMILIES = ("tail_sweep", "two_shares", "includes", "long_tail", "window_fit", "tampered")


class Case:
    """One block: its bincode, the StatementBlock it was built from (None for a tampered one), the
    status the construction intends, and what the families are indexed by (tail, L = the share's
    payload bytes, d = the start alignment and value = the fit test's left side for window_fit)."""

    def __init__(self, family, name, bincode, block, status, **attrs):
        self.family, self.name, self.bincode, self.block, self.status = family, name, bincode, block, status
        self.tail, self.L, self.d, self.value = (attrs.get(k) for k in ("tail", "L", "d", "value"))
        self.variant = attrs.get("variant")

    def __repr__(self):
        return f"<{self.family}: {self.name}>"


def committee():
    """(pks, stakes, epoch) of the corpus' committee."""
    pks = np.frombuffer(b"".join(O.public_key(B.authority_seed(a)) for a in range(N_AUTH)), dtype=np.uint8)
    return pks.reshape(-1, 32), np.array(STAKES, dtype=np.uint64), EPOCH


def payload(n, *salt):
    return hashlib.shake_256(repr(salt).encode()).digest(n) if n else b""


def pieces(block):
    """[(kind, start, end)] of the block's pre-image, in the units a piece-by-piece walk emits: the
    header, each include, a Share's tag byte and its payload 64 bytes at a time, a vote (its first
    locator), a Reject(Some)'s second locator, a VoteRange, the metadata."""
    out, pos = [], 0

    def add(kind, n):
        nonlocal pos
        out.append((kind, pos, pos + n))
        pos += n

    # the header is a reference's authority and round without its digest; an empty block's
    # pre-image is the header and the metadata
    ref = len(B.BlockReference(0, 0, bytes(32)).preimage())
    header = ref - 32
    meta = len(B.StatementBlock(block.authority, block.round, [], [], block.meta_creation_time_ns, block.epoch_marker,
                                block.epoch).preimage()) - header
    add("header", header)
    for _ in block.includes:
        add("include", ref)
    for s in block.statements:
        n = len(B.statement_preimage(s))
        if s[0] == "share":
            add("share_tag", n - len(s[1]))
            for lo in range(0, len(s[1]), 64):
                add("share_sub", min(64, len(s[1]) - lo))
        elif s[0] == "reject" and s[2] is not None:
            second = len(s[2].preimage())
            add("vote", n - second)
            add("second_locator", second)
        elif s[0] == "range":
            add("range", n)
        else:
            add("vote", n)
    add("metadata", meta)
    assert pos == len(block.preimage())
    return out


class _Builder:
    def __init__(self):
        self.seeds = [B.authority_seed(a) for a in range(N_AUTH)]
        self.gen = [B.genesis(a, EPOCH) for a in range(N_AUTH)]
        self.n = 0
        self.out = []

    def tail(self, kind):
        loc = B.Locator(self.gen[3].reference(), 7)
        other = B.Locator(self.gen[5].reference(), 2**40 + 9)
        return {"none": [], "accept": [("accept", loc)], "reject": [("reject", loc, None)],
                "reject_some": [("reject", loc, other)], "range": [("range", self.gen[4].reference(), 3, 11)]}[kind]

    def block(self, n_inc, statements, round_=1):
        """A block of the next author in turn; includes: the genesis blocks of authorities 0..n_inc-1."""
        author = self.n % N_AUTH
        self.n += 1
        inc = [self.gen[a].reference() for a in range(n_inc)]
        return B.new_with_signer(author, round_, inc, statements, (self.n << 64) + 10**8 + self.n, bool(self.n & 1),
                                 EPOCH, self.seeds[author], O.sign)

    def add(self, family, what, blk, status=OK, **attrs):
        name = f"{family}: {what} |P|%128={len(blk.preimage()) % 128}"
        self.out.append(Case(family, name, blk.bincode(), blk, status, **attrs))
        return self.out[-1]


def _share_for(residue, tail_bytes, at_least):
    """The smallest Share payload >= at_least for which a one-include block with that tail has
    |P| % 128 == residue."""
    fixed = len(B.StatementBlock(0, 1, [B.BlockReference(0, 0, bytes(32))], [("share", b"")], 0, False, 0).preimage())
    return at_least + (residue - fixed - tail_bytes - at_least) % 128


def _tamper(case):
    """The three variants of a clean block: P's last byte flipped under the stale digest, the first
    byte of the signature's s flipped with the digest recomputed, the bincode cut by one byte."""
    b, blk = case.bincode, case.block
    # P ends with the epoch (big-endian): its last byte is the epoch's low byte, which bincode holds
    # ahead of the epoch's other 7 bytes, the signature's length word and the signature
    at = len(b) - 64 - 8 - 8
    assert blk.preimage()[-1] == b[at]
    stale = b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
    sig = bytearray(blk.signature)
    sig[32] ^= 1
    bad = B.StatementBlock(blk.authority, blk.round, blk.includes, blk.statements, blk.meta_creation_time_ns,
                           blk.epoch_marker, blk.epoch, bytes(sig))
    bad.digest = bad.compute_digest()
    return [("last byte of P flipped", stale, DIGEST_MISMATCH), ("first byte of s flipped", bad.bincode(), SIG_INVALID),
            ("cut by one byte", b[:-1], PARSE_ERROR)]


@functools.lru_cache(maxsize=None)
def corpus():
    """[Case], in a fixed order: the families of FAMILIES one after another."""
    bd = _Builder()
    # tail_sweep: |P| = 90 + L + tail, so L = 0..255 takes |P| % 128 through every value twice, the
    # second time half a 128-byte block further into the Share's 64-byte steps
    for tail in TAILS:
        for L in range(256):
            blk = bd.block(1, [("share", payload(L, tail, L))] + bd.tail(tail))
            bd.add("tail_sweep", f"tail={tail} L={L}", blk, tail=tail, L=L)
    sweep = list(bd.out)
    # two_shares: the second Share's tag byte at every position of a block (alone at 127 for a = 62),
    # the first one empty (a = 0) or ending on a boundary (a = 63)
    for a in range(131):
        blk = bd.block(1, [("share", payload(a, "first", a)), ("share", payload(TWO_SHARES_TOTAL - a, "second", a))])
        bd.add("two_shares", f"Share({a}) Share({TWO_SHARES_TOTAL - a})", blk, L=a)
    # includes: 0 (round 0: GENESIS) and 1..9, followed at once by the metadata, a Share or a VoteRange
    for a in (0, 7):
        bd.out.append(Case("includes", f"includes: genesis of authority {a} |P|%128=41", bd.gen[a].bincode(), bd.gen[a],
                           GENESIS, tail="none", L=None))
    bd.add("includes", "k=0 round 0 signed Share(70)", bd.block(0, [("share", payload(70, "g"))], round_=0), GENESIS,
           tail="none", L=70)
    for k in range(1, N_AUTH):
        for what, sts in (("no statements", []), ("Share(5)", [("share", payload(5, "inc", k))]), ("range", bd.tail("range"))):
            bd.add("includes", f"k={k} {what}", bd.block(k, sts), tail="none", L=len(sts[0][1]) if what[0] == "S" else None)
    # long_tail: many common blocks before P ends
    for at_least in (1024, 9000):
        for tail in TAILS:
            tb = sum(len(B.statement_preimage(s)) for s in bd.tail(tail))
            for res in RESIDUES:
                L = _share_for(res, tb, at_least)
                blk = bd.block(1, [("share", payload(L, "long", tail, L))] + bd.tail(tail))
                assert len(blk.preimage()) % 128 == res
                bd.add("long_tail", f"tail={tail} L={L}", blk, tail=tail, L=L)
    # window_fit: the bincode length set through the Share; d is the alignment the block is to be placed at
    base = len(bd.block(1, [("share", b"")]).bincode())
    bd.n -= 1
    for d in range(8):
        for value in FIT_VALUES:
            L = value - 16 - d - base
            blk = bd.block(1, [("share", payload(L, "fit", d, value))])
            assert d + len(blk.bincode()) + 16 == value
            bd.add("window_fit", f"d={d} d+len+16={value} L={L}", blk, L=L, d=d, value=value)
    for value in FIT_VALUES:  # the host's eligibility rule for the online service: len + 32 <= window
        L = value - 32 - base
        blk = bd.block(1, [("share", payload(L, "fit32", value))])
        assert len(blk.bincode()) + 32 == value
        bd.add("window_fit", f"len+32={value} L={L}", blk, L=L, d=None, value=value)
    # tampered: one block per residue (the tails in turn), three variants each
    for i, res in enumerate(TAMPER_RESIDUES):
        src = next(c for c in sweep if c.tail == TAILS[i % len(TAILS)] and len(c.block.preimage()) % 128 == res)
        for what, b, status in _tamper(src):
            bd.out.append(Case("tampered", f"tampered: {what}, of {src.name}", b, None, status, tail=src.tail, L=src.L,
                               variant=what))
    return tuple(bd.out)


def family(*names):
    return [c for c in corpus() if c.family in names]


@functools.lru_cache(maxsize=None)
def oracle_results():
    """{case name: (status, message digest, block digest)} from the C oracle, computed once."""
    cases = corpus()
    st, md, bd = oracle_verify([c.bincode for c in cases])
    return {c.name: (int(st[i]), md[i].tobytes(), bd[i].tobytes()) for i, c in enumerate(cases)}


def oracle_verify(bins):
    """(status, md, bd) arrays of the C oracle's StatementBlock::verify over bincodes."""
    pks, stakes, epoch = committee()
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(len(bins), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    return O.block_verify_batch(np.frombuffer(b"".join(bins) + b"\0", dtype=np.uint8), offs, lens, pks, stakes, epoch)


def golden_summary():
    """What tests/golden/preimage_edges.json holds."""
    cases, res = corpus(), oracle_results()
    sha = lambda k: hashlib.sha256(b"".join(res[c.name][k] for c in cases if res[c.name][0] != PARSE_ERROR)).hexdigest()
    return {"blocks": len(cases), "sha256_bincode_concat": hashlib.sha256(b"".join(c.bincode for c in cases)).hexdigest(),
            "sha256_msg_digests": sha(1), "sha256_block_digests": sha(2),
            "tampered_status": [res[c.name][0] for c in cases if c.family == "tampered"]}
