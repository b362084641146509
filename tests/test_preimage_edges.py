"""CPU: the corpus of tests/preimage_edges.py covers what it says it covers, and the two references
the GPU tests lean on agree on it: the C oracle's StatementBlock::verify (oracle/block.c) and
hashlib's Blake2b over the Python builder's pre-image (oracle/blocks.py). The lists of positions
below are worked out here from the format's sizes, not taken from the corpus or from a kernel."""
import collections
import hashlib

import pytest

import blocks as B
import preimage_edges as PE


@pytest.fixture(scope="module")
def clean():
    return [c for c in PE.corpus() if c.block is not None]


@pytest.fixture(scope="module")
def splits(clean):
    """{piece kind: {(pos_before, pos_after)}}: where in its 128-byte block each piece starts, and
    where the write position stands after it (above 128: the piece straddles a boundary)."""
    out = collections.defaultdict(set)
    for c in clean:
        for kind, lo, hi in PE.pieces(c.block):
            out[kind].add((lo % 128, lo % 128 + hi - lo))
    return out


def test_names_are_unique_and_families_in_order():
    cases = PE.corpus()
    assert len({c.name for c in cases}) == len(cases)
    seen = [c.family for c in cases]
    assert [f for i, f in enumerate(seen) if i == 0 or seen[i - 1] != f] == list(PE.FAMILIES)
    sizes = collections.Counter(seen)
    assert sizes["tail_sweep"] == 256 * len(PE.TAILS) and sizes["two_shares"] == 131
    assert sizes["tampered"] == 3 * len(PE.TAMPER_RESIDUES)


def test_piece_sizes_are_the_formats(clean):
    """The piece sizes, from oracle/blocks.py's encoding of one block that holds every kind."""
    ref = B.BlockReference(1, 2, bytes(32))
    loc = B.Locator(ref, 3)
    blk = B.StatementBlock(0, 1, [ref], [("share", bytes(70)), ("accept", loc), ("reject", loc, None), ("reject", loc, loc),
                                         ("range", ref, 0, 1)], 5, False, 0)
    assert [(k, hi - lo) for k, lo, hi in PE.pieces(blk)] == [
        ("header", 16), ("include", 48), ("share_tag", 1), ("share_sub", 64), ("share_sub", 6), ("vote", 57), ("vote", 57),
        ("vote", 57), ("second_locator", 56), ("range", 65), ("metadata", 25)]
    for c in clean[::97]:
        ps = PE.pieces(c.block)
        assert ps[0][1] == 0 and all(a[2] == b[1] for a, b in zip(ps, ps[1:])) and ps[-1][2] == len(c.block.preimage())


@pytest.mark.parametrize("tail", PE.TAILS)
def test_every_residue_for_every_tail_twice(tail):
    """tail_sweep: one include, Share(L) for L = 0..255, the tail: |P| % 128 takes every value twice,
    the second time one 128-byte block (two more 64-byte steps of the payload) later."""
    kinds = {"none": [], "accept": ["accept"], "reject": ["reject"], "reject_some": ["reject"], "range": ["range"]}[tail]
    by_res = collections.defaultdict(list)
    for c in PE.family("tail_sweep"):
        if c.tail == tail:
            assert len(c.block.includes) == 1 and [s[0] for s in c.block.statements] == ["share"] + kinds
            assert tail not in ("reject", "reject_some") or (c.block.statements[1][2] is not None) == (tail == "reject_some")
            assert len(c.block.statements[0][1]) == c.L
            by_res[len(c.block.preimage()) % 128].append(c.L)
    assert sorted(by_res) == list(range(128))
    for res, ls in by_res.items():
        assert len(ls) == 2 and ls[1] - ls[0] == 128, (tail, res, ls)


def test_signature_schedules(clean):
    """|P| % 128 of 0 (a full last block), 1..64 (P || sig ends in P's last block; at 64 on its
    boundary) and 65..127 (one block more) all occur, with 0, 1 and many blocks before the last."""
    kinds = collections.defaultdict(set)
    for c in clean:
        n = len(c.block.preimage())
        r = n % 128
        kinds["full" if r == 0 else "fits" if r < 64 else "ends on" if r == 64 else "straddles"].add(min((n - 1) // 128, 9))
    for k in ("full", "fits", "ends on", "straddles"):
        assert {1, 2, 9} <= kinds[k], (k, kinds[k])  # whole blocks ahead of P's last one (9: nine or more)
    assert 0 in kinds["fits"]  # the genesis block: P || sig in one block


def test_include_splits(splits):
    """An include is 48 bytes at 16 + 48 k: with up to 9 of them, every offset k = 0..8 allows, of
    which k = 2 and 7 straddle, k = 4 ends on a boundary and k = 5 starts on one."""
    want = {((16 + 48 * k) % 128, (16 + 48 * k) % 128 + 48) for k in range(9)}
    assert want <= splits["include"]
    assert {(112, 160), (96, 144), (80, 128), (0, 48)} <= want


def test_share_splits(splits):
    # the tag byte alone at the end of a block, and opening one
    assert {(127, 128), (0, 1)} <= splits["share_tag"]
    # a whole 64-byte step from every position at which it straddles (65..127), ends on (64) or
    # starts on (0) a boundary
    assert {(p, p + 64) for p in list(range(64, 128)) + [0]} <= splits["share_sub"]
    # the payload's last, partial step completing a block with a length that is no multiple of 8
    # (the step is written in whole 8-byte words), and straddling one
    partial = {(lo, hi) for lo, hi in splits["share_sub"] if hi - lo < 64}
    assert any(hi == 128 and (hi - lo) % 8 for lo, hi in partial)
    assert any(hi > 128 and (hi - lo) % 8 for lo, hi in partial)
    assert {hi - lo for lo, hi in partial} == set(range(1, 64))


@pytest.mark.parametrize("kind,size", [("vote", 57), ("second_locator", 56), ("range", 65), ("metadata", 25)])
def test_fixed_piece_splits(splits, kind, size):
    """Votes, a Reject(Some)'s second locator, VoteRanges and the metadata follow a Share of any
    length, so each starts at every position of a block: every straddle, ending on and starting on."""
    assert {(p, p + size) for p in range(128)} <= splits[kind]


def test_two_shares():
    cases = PE.family("two_shares")
    assert [c.L for c in cases] == list(range(131))
    for c in cases:
        a, b = (len(s[1]) for s in c.block.statements)
        assert a == c.L and a + b == PE.TWO_SHARES_TOTAL
    tag2 = {PE.pieces(c.block)[3 + -(-c.L // 64)][1] for c in cases}  # header, include, tag, the first payload's steps
    assert {126, 127, 128, 129} <= tag2 and all(PE.pieces(c.block)[3 + -(-c.L // 64)][0] == "share_tag" for c in cases)


def test_includes_family():
    cases = PE.family("includes")
    assert {len(c.block.includes) for c in cases} == set(range(10))
    assert {c.status for c in cases if not c.block.includes} == {PE.GENESIS}
    assert all(c.status == PE.OK for c in cases if c.block.includes)
    for k in range(1, 10):  # the metadata, a Share and a VoteRange each right behind the k-th include
        assert {(c.block.statements or [("meta",)])[0][0] for c in cases if len(c.block.includes) == k} == {"meta", "share", "range"}


def test_long_tail_family():
    got = collections.defaultdict(set)
    for c in PE.family("long_tail"):
        n = len(c.block.preimage())
        got[(c.tail, n % 128)].add("1k" if 1024 <= n < 1500 else "9k" if 9000 <= n < 9500 else "?")
        assert len(c.bincode) + 32 <= PE.WINDOW  # the online service still takes it
    assert got == {(t, r): {"1k", "9k"} for t in PE.TAILS for r in PE.RESIDUES}


def test_window_fit_family():
    cases = PE.family("window_fit")
    assert {(c.d, c.value) for c in cases} == {(d, v) for d in list(range(8)) + [None] for v in PE.FIT_VALUES}
    for c in cases:
        assert (c.d + len(c.bincode) + 16 if c.d is not None else len(c.bincode) + 32) == c.value, c.name


def test_tampered_family(golden):
    cases = PE.family("tampered")
    res = PE.oracle_results()
    assert [c.status for c in cases] == [PE.DIGEST_MISMATCH, PE.SIG_INVALID, PE.PARSE_ERROR] * len(PE.TAMPER_RESIDUES)
    assert [res[c.name][0] for c in cases] == [c.status for c in cases] == golden("preimage_edges.json")["tampered_status"]
    by_name = {c.name: c for c in PE.corpus()}
    srcs = [by_name[c.name.split(", of ", 1)[1]] for c in cases[::3]]
    assert [len(s.block.preimage()) % 128 for s in srcs] == list(PE.TAMPER_RESIDUES)
    assert len({s.tail for s in srcs}) == len(PE.TAILS)
    for c, s in zip(cases[::3], srcs):  # the stale-digest variant differs in P's last byte alone
        diff = [i for i in range(len(s.bincode)) if s.bincode[i] != c.bincode[i]]
        assert len(diff) == 1 and len(c.bincode) == len(s.bincode)


def test_oracle_and_builder_agree(clean):
    """The C oracle accepts every clean block (GENESIS for round 0), and its two digests are
    hashlib's Blake2b-256 over the Python builder's P and P || sig."""
    res = PE.oracle_results()
    for c in clean:
        st, md, bd = res[c.name]
        assert st == c.status, c.name
        p = c.block.preimage()
        assert md == hashlib.blake2b(p, digest_size=32).digest(), c.name
        assert bd == hashlib.blake2b(p + c.block.signature, digest_size=32).digest() == c.block.digest, c.name
    assert sum(1 for c in clean if c.status == PE.OK) == len(clean) - 3


def test_golden(golden):
    assert PE.golden_summary() == golden("preimage_edges.json")
