"""Helper (not a test): the include checks and the threshold clock at the end of
StatementBlock::verify, restated in plain Python from the reference's text, and the blocks that
pin them at the committee's edges.

  StatementBlock::verify   types.rs:339-375: unknown author, genesis, signature, then per include
                           in list order known_authority before round < own round, then
                           VoteRange::verify per statement (types.rs:440-460), then the clock
  threshold clock          threshold_clock.rs:12-35: the includes of round r-1 go into a
                           StakeAggregator, which holds a *set* of authorities
                           (committee.rs:314-320): each one counts once
  committee                committee.rs:50-57: total = checked sum of the stakes, quorum threshold
                           = 2 * total / 3; committee.rs:125-127: quorum iff stake > threshold

verdict() uses Python integers and a set(); it shares nothing with oracle/block.c or the library's
block_codec.cpp. quorum_cases() builds signed blocks (oracle/blocks.py) with verdict()'s answer."""
import hashlib

import blocks as B
import oracle as O

(OK, PARSE_ERROR, DIGEST_MISMATCH, EPOCH_MISMATCH, UNKNOWN_AUTHOR, GENESIS, SIG_INVALID, INCLUDE_UNKNOWN_AUTHORITY,
 INCLUDE_ROUND, VOTE_RANGE, THRESHOLD_CLOCK, VOTE_RANGE_TOO_LONG, VOTE_RANGE_END_TOO_LARGE) = range(13)
NAMES = ["OK", "PARSE_ERROR", "DIGEST_MISMATCH", "EPOCH_MISMATCH", "UNKNOWN_AUTHOR", "GENESIS", "SIG_INVALID",
         "INCLUDE_UNKNOWN_AUTHORITY", "INCLUDE_ROUND", "VOTE_RANGE", "THRESHOLD_CLOCK", "VOTE_RANGE_TOO_LONG",
         "VOTE_RANGE_END_TOO_LARGE"]
U64 = 1 << 64
MAX_RANGE = 1024 * 1024


# ---- the model -------------------------------------------------------------------------------
def quorum_threshold(stakes):
    total = 0
    for s in stakes:
        total += s
        if total >= U64:  # checked_add(..).expect("Total stake overflow")
            raise OverflowError("total stake overflow")
    if 2 * total >= U64:  # 2 * total_stake in u64
        raise OverflowError("2 * total stake overflow")
    return 2 * total // 3


def verdict(author, round_, includes, stakes, sig_valid, ranges=()):
    """The MV_BLOCK_* status of a block whose digest and epoch are right. includes: (authority,
    round) in list order; ranges: (start, end) of its VoteRange statements in order."""
    n = len(stakes)
    if not author < n:
        return UNKNOWN_AUTHOR
    if round_ == 0:
        return GENESIS
    if not sig_valid:
        return SIG_INVALID
    for a, r in includes:
        if not a < n:
            return INCLUDE_UNKNOWN_AUTHORITY
        if not r < round_:
            return INCLUDE_ROUND
    for start, end in ranges:
        if not end >= start:
            return VOTE_RANGE
        if not end - start < MAX_RANGE:
            return VOTE_RANGE_TOO_LONG
        if not end < MAX_RANGE:
            return VOTE_RANGE_END_TOO_LARGE
    threshold = quorum_threshold(stakes)
    votes, stake, is_quorum = set(), 0, False
    for a, r in includes:
        if r == round_ - 1:
            if a not in votes:
                votes.add(a)
                stake += stakes[a]
            is_quorum = stake > threshold
    return OK if is_quorum else THRESHOLD_CLOCK


# ---- committees ------------------------------------------------------------------------------
def _about_2p60():
    # total 18m + 1 just under 2^63; 2 * total // 3 = 12m = (4m + 2) + (4m - 2) + 4m: three keys sit
    # exactly on the threshold
    m = (2**63 - 1) // 18 - 5
    return [4 * m + 2, 3 * m, 4 * m - 2, 3 * m + 1, 4 * m]


COMMITTEES = {
    "n1": [1], "n2": [1] * 2, "n3": [1] * 3, "n4": [1] * 4,
    "n7_total10": [3, 1, 1, 2, 1, 1, 1],
    "n33": [1] * 33, "n128": [1] * 128, "n129": [1] * 129, "n512": [1] * 512,
    "n100_2p40": [2**40 + i for i in range(100)],
    "n5_2p60": _about_2p60(),
    "n4_whale": [2**62, 1, 1, 1],
}
FIRST_FAILURE_IN = ("n7_total10", "n129")  # the 130-include blocks
MANY_INCLUDES = {"n7_total10": (64, 65, 128), "n129": (64, 65, 128, 513, 700), "n512": (513, 700)}


def committee_keys(n):
    return [O.public_key(B.authority_seed(a)) for a in range(n)]


# ---- the cases -------------------------------------------------------------------------------
class Case:
    def __init__(self, note, block, status):
        self.note, self.bincode, self.status = note, block.bincode(), status


def _dig(*what):
    return hashlib.blake2b(repr(what).encode(), digest_size=32).digest()


def _exact_set(stakes, thr):
    """Authorities whose stake is exactly thr, or None: arithmetic for equal stakes, every subset
    of a small committee."""
    n = len(stakes)
    if len(set(stakes)) == 1:
        return list(range(thr // stakes[0])) if thr % stakes[0] == 0 else None
    if n <= 12:
        for m in range(1 << n):
            if sum(stakes[a] for a in range(n) if m >> a & 1) == thr:
                return [a for a in range(n) if m >> a & 1]
    return None


def _short_set(stakes, thr, without=(), descending=False):
    """Authorities taken in index order while the stake stays <= thr."""
    out, s = [], 0
    for a in (reversed(range(len(stakes))) if descending else range(len(stakes))):
        if a not in without and s + stakes[a] <= thr:
            out.append(a)
            s += stakes[a]
    return out


def quorum_cases(n_auth, stakes):
    """[Case]: signed blocks for the committee of n_auth keys (B.authority_seed) with these stakes."""
    assert len(stakes) == n_auth
    seeds = {}
    out = []
    thr = quorum_threshold(stakes)
    stake_of = lambda s: sum(stakes[a] for a in set(s))

    def add(note, includes, author=0, round_=5, sig_valid=True, ranges=()):
        """includes: (authority, round); each gets a digest of its own."""
        refs = [B.BlockReference(a, r, _dig(note, k, a, r)) for k, (a, r) in enumerate(includes)]
        sts = [("share", bytes([len(out) & 0xFF]) * 8)]
        sts += [("range", B.BlockReference(0, 1, _dig(note, "range", k)), s, e) for k, (s, e) in enumerate(ranges)]
        signer = author % n_auth  # (an unknown author has no key: any signature will do)
        if signer not in seeds:
            seeds[signer] = B.authority_seed(signer)
        b = B.new_with_signer(author, round_, refs, sts, 10**8 * (round_ % 1000) + len(out), False, 0, seeds[signer],
                              O.sign)
        if not sig_valid:  # one bit of s flipped, the digest recomputed over the new signature
            sig = bytearray(b.signature)
            sig[40] ^= 0x10
            b.signature = bytes(sig)
            b.digest = b.compute_digest()
        out.append(Case(note, b, verdict(author, round_, includes, stakes, sig_valid, ranges)))
        return out[-1]

    at = lambda auths, r: [(a, r) for a in auths]
    exact = _exact_set(stakes, thr)
    below = exact if exact is not None else _short_set(stakes, thr)
    how = "exactly 2*total//3" if exact is not None else "the most that fits under 2*total//3"
    rest = [a for a in range(n_auth) if a not in below]
    nxt = min(rest, key=lambda a: (stakes[a], a))  # the lightest authority left
    quorum = below + [nxt]
    assert stake_of(below) <= thr < stake_of(quorum)

    # quorum boundaries
    c = add(f"boundary: round-4 stake {how}", at(below, 4))
    assert c.status == THRESHOLD_CLOCK
    c = add("boundary: the same set plus the lightest authority left", at(quorum, 4))
    assert c.status == OK
    add("boundary: no includes", [])
    c = add("boundary: all n authorities", at(range(n_auth), 4))
    assert c.status == OK

    # duplicates
    heavy = max(range(n_auth), key=lambda a: (stakes[a], -a))
    add("duplicates: the heaviest authority three times, three digests", at([heavy] * 3, 4))
    add("duplicates: authority n-1 three times among old rounds", [(n_auth - 1, 4), (0, 3), (n_auth - 1, 4), (0, 0), (n_auth - 1, 4)])
    if below:
        h = max(below, key=lambda a: (stakes[a], -a))
        c = add("duplicates: one short of quorum plus its heaviest member again", at(below + [h], 4))
        assert c.status == THRESHOLD_CLOCK
        c = add("duplicates: one short of quorum, its heaviest member first and last", at([h] + [a for a in below if a != h] + [h], 4))
        assert c.status == THRESHOLD_CLOCK
        # the duplicate more than 64 positions after the original: old-round includes between
        gap = at([k % n_auth for k in range(max(0, 66 - len(below)))], 3)
        c = add("duplicates: the heaviest member again more than 64 includes later",
                [(h, 4)] + gap + at([a for a in below if a != h], 4) + [(h, 4)])
        assert c.status == THRESHOLD_CLOCK
        c = add("duplicates: every member of a short set twice, then the deciding authority", at(below + below + [nxt], 4))
        assert c.status == OK

    # rounds that do not count
    c = add("old rounds: every authority at rounds 3 and 0, too few at round 4",
            at(range(n_auth), 3) + at(below, 4) + at(range(n_auth), 0))
    assert c.status == THRESHOLD_CLOCK
    add("old rounds: a quorum at round 3 only", at(quorum, 3))

    # bitmap edges: the deciding authority comes last
    for d in sorted({0, 31, 32, 63, 64, 127, 128, 511, n_auth - 1}):
        if d >= n_auth:
            continue
        s = _short_set(stakes, thr, without=(d,), descending=True)  # high words of the bitmap first
        if stake_of(s) + stakes[d] <= thr:
            s = _short_set(stakes, thr, without=(d,))
        if stake_of(s) + stakes[d] <= thr:
            continue  # this key cannot decide in this committee
        c = add(f"bitmap: one short without authority {d}", at(s, 4))
        assert c.status == THRESHOLD_CLOCK
        c = add(f"bitmap: authority {d} is the last one needed", at(s + [d], 4))
        assert c.status == OK

    # own round 1
    c = add("round 1: a quorum of round-0 includes", at(quorum, 0), round_=1)
    assert c.status == OK
    add("round 1: one short at round 0", at(below, 0), round_=1)
    add("round 0: genesis does not go through verify", [], round_=0)

    # 64-bit fields
    big = 2**32 + 5
    c = add("64-bit: own round 2^32+5, parents at 2^32+4", at(quorum, big - 1), round_=big)
    assert c.status == OK
    c = add("64-bit: own round 2^32+5, the deciding parent at round 4", at(below, big - 1) + [(nxt, 4)], round_=big)
    assert c.status == THRESHOLD_CLOCK
    c = add("64-bit: own round 2^32+5, every parent at round 4", at(quorum, 4), round_=big)
    assert c.status == THRESHOLD_CLOCK
    c = add("64-bit: own round 5, parents at round 2^32+4", at(quorum, big - 1))
    assert c.status == INCLUDE_ROUND
    c = add("64-bit: an include at round 2^33 under own round 2^32+5", at(quorum, big - 1) + [(0, 2**33)], round_=big)
    assert c.status == INCLUDE_ROUND
    c = add("64-bit: an include at round 2^64-1", at(quorum, 4) + [(0, U64 - 1)])
    assert c.status == INCLUDE_ROUND
    for a in (2**32, 2**32 + 1, U64 - 1):
        c = add(f"64-bit: include authority {a}", at(quorum, 4) + [(a, 4)])
        assert c.status == INCLUDE_UNKNOWN_AUTHORITY
    c = add("64-bit: block author 2^32", at(quorum, 4), author=2**32)
    assert c.status == UNKNOWN_AUTHOR
    add("author n", at(quorum, 4), author=n_auth)
    c = add("64-bit: own round 2^64-1, parents at 2^64-2", at(quorum, U64 - 2), round_=U64 - 1)
    assert c.status == OK
    add("64-bit: own round 2^64-1, one short at 2^64-2", at(below, U64 - 2), round_=U64 - 1)

    # precedence
    c = add("precedence: include round == own round, no quorum", at(below, 4) + [(0, 5)])
    assert c.status == INCLUDE_ROUND
    c = add("precedence: include authority n, no quorum", [(n_auth, 4)] + at(below, 4))
    assert c.status == INCLUDE_UNKNOWN_AUTHORITY
    c = add("precedence: bad signature, a failing include, no quorum", at(below, 4) + [(n_auth, 9)], sig_valid=False)
    assert c.status == SIG_INVALID
    add("precedence: bad signature on a quorum", at(quorum, 4), sig_valid=False)
    c = add("precedence: VoteRange end < start, no quorum", at(below, 4), ranges=[(0, 3), (5, 4)])
    assert c.status == VOTE_RANGE
    c = add("precedence: a failing include before a failing VoteRange", at(quorum, 4) + [(0, 6)], ranges=[(5, 4)])
    assert c.status == INCLUDE_ROUND
    add("precedence: a good VoteRange, no quorum", at(below, 4), ranges=[(0, 3)])

    name = next((k for k, v in COMMITTEES.items() if v == list(stakes)), None)
    # first failure decides, over more than 64 includes (130 of them; a quorum at round 4 or not)
    if name in FIRST_FAILURE_IN:
        def long_list(bad):
            inc = [(quorum[k % len(quorum)], 4) for k in range(130)]
            for pos, what in bad.items():
                inc[pos] = {"auth": (n_auth, 4), "round": (0, 5), "both": (n_auth + 7, 5)}[what]
            return inc

        for note, bad, want in [
            ("round at 70, unknown authority at 5", {70: "round", 5: "auth"}, INCLUDE_UNKNOWN_AUTHORITY),
            ("unknown authority at 70, round at 5", {70: "auth", 5: "round"}, INCLUDE_ROUND),
            ("round at 64, unknown authority at 65 and 129", {64: "round", 65: "auth", 129: "auth"}, INCLUDE_ROUND),
            ("unknown authority at 64, round at 65 and 129", {64: "auth", 65: "round", 129: "round"}, INCLUDE_UNKNOWN_AUTHORITY),
            ("unknown authority at 65, round at 129", {65: "auth", 129: "round"}, INCLUDE_UNKNOWN_AUTHORITY),
            ("round at 65, unknown authority at 129", {65: "round", 129: "auth"}, INCLUDE_ROUND),
            ("round at 63, unknown authority at 64 (two lanes' first)", {63: "round", 64: "auth"}, INCLUDE_ROUND),
            ("one include at 100 both unknown and at a bad round", {100: "both"}, INCLUDE_UNKNOWN_AUTHORITY),
            ("round at 129 only", {129: "round"}, INCLUDE_ROUND),
        ]:
            c = add(f"first failure of 130: {note}", long_list(bad))
            assert c.status == want

    # many includes: duplicates and old rounds mixed in, the deciding authority last
    for count in MANY_INCLUDES.get(name, ()):
        for members, tag in ((quorum, "a quorum"), (below, "one short")):
            body = list(below)[:count - 1]  # (more members than places: whatever fits)
            slots = count - 1
            where = {j * slots // len(body): a for j, a in enumerate(body)}  # the members spread over the list
            inc = []
            for k in range(slots):
                if k in where:
                    inc.append((where[k], 4))
                else:  # a duplicate, a round-3 and a round-0 include in turn
                    inc.append([(body[k % len(body)], 4), ((k * 7) % n_auth, 3), ((k * 13) % n_auth, 0)][k % 3])
            inc.append((nxt, 4) if members is quorum else (body[-1], 4))
            assert len(inc) == count
            add(f"many includes: {count}, {tag}", inc)
    return out
