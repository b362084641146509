"""Blocks for the vote-aggregation tests: a bincode builder for Data<StatementBlock> (types.rs:93-114)
with statements in any interleaving, and seeded random sequences. Nothing is signed: mv_aggregate_votes
does not verify.

A reference is (authority, round, digest32). A statement is one of
    ("share", payload)                      BaseStatement::Share
    ("vote", ref, offset)                   Vote(locator, Accept)
    ("reject", ref, offset, None | (ref2, offset2))   Vote(locator, Reject(Option<locator>))
    ("range", ref, start, end)              VoteRange
A block is (author, ref, statements); its bytes come from encode().
"""
import random
import struct

U64 = (1 << 64) - 1


def digest(tag) -> bytes:
    """A 32-byte digest that tells blocks apart (all eight-byte words differ by tag)."""
    r = random.Random(f"votes-digest-{tag}")
    return bytes(r.getrandbits(8) for _ in range(32))


def ref_of(author: int, rnd: int, tag=None):
    return (author, rnd, digest((author, rnd, tag)))


def _ref(r) -> bytes:
    return struct.pack("<QQQ", r[0], r[1], 32) + r[2]


def ref_words(r):
    return (r[0], r[1]) + struct.unpack("<4Q", r[2])


def encode(ref, statements, includes=()) -> bytes:
    out = [_ref(ref), struct.pack("<Q", len(includes))]
    out += [_ref(i) for i in includes]
    out.append(struct.pack("<Q", len(statements)))
    for st in statements:
        if st[0] == "share":
            out.append(struct.pack("<IQ", 0, len(st[1])) + st[1])
        elif st[0] == "vote":
            out.append(struct.pack("<I", 1) + _ref(st[1]) + struct.pack("<QI", st[2] & U64, 0))
        elif st[0] == "reject":
            out.append(struct.pack("<I", 1) + _ref(st[1]) + struct.pack("<QI", st[2] & U64, 1))
            if st[3] is None:
                out.append(b"\0")
            else:
                out.append(b"\1" + _ref(st[3][0]) + struct.pack("<Q", st[3][1]))
        elif st[0] == "range":
            out.append(struct.pack("<I", 2) + _ref(st[1]) + struct.pack("<QQ", st[2] & U64, st[3] & U64))
        else:
            raise ValueError(st[0])
    out.append(struct.pack("<QQBQQ", 0, 0, 0, 0, 64) + bytes(64))
    return b"".join(out)


def block(author: int, rnd: int, statements, tag=None):
    return (author, ref_of(author, rnd, tag), list(statements))


def encode_block(b) -> bytes:
    return encode(b[1], b[2])


def shares(k: int):
    return [("share", b"tx%d" % i) for i in range(k)]


def unequal_stakes(n: int):
    return [1 + (i * 7) % 5 for i in range(n)]


def quorum(stakes) -> int:
    return 2 * sum(stakes) // 3 + 1  # committee.rs:56-57, :79-81


def random_blocks(seed: int, n_auth: int, n_blocks: int):
    """Sharing blocks with Shares interleaved with votes, and ranges over earlier, unseen and partly
    certified blocks that overlap, split and straddle earlier ranges; now and then a block again."""
    r = random.Random(seed)
    made, out = [], []
    for k in range(n_blocks):
        if made and r.random() < 0.06:
            out.append(r.choice(made))
            continue
        author = r.randrange(n_auth)
        sts = []
        for _ in range(r.randrange(0, 12)):
            x = r.random()
            if x < 0.4:
                sts.append(("share", bytes([r.randrange(256)]) * r.randrange(0, 5)))
                continue
            tgt = r.choice(made[-3:])[1] if made and r.random() < 0.9 else ref_of(r.randrange(n_auth), 99, r.randrange(4))
            if x < 0.55:
                sts.append(("vote", tgt, r.randrange(0, 10)))
            elif x < 0.6:
                sts.append(("reject", tgt, r.randrange(0, 10), None if r.random() < 0.5 else (tgt, 1)))
            elif x < 0.63:
                sts.append(("vote", tgt, U64))
            elif x < 0.66:
                s = r.randrange(0, 10)
                sts.append(("range", tgt, s, s - r.randrange(0, 3)))
            else:
                s = r.randrange(0, 4)
                sts.append(("range", tgt, s, s + r.randrange(0, 10)))
        b = block(author, 1 + k, sts, tag=(seed, k))  # (references differ from sequence to sequence)
        made.append(b)
        out.append(b)
    return out


# ---------------------------------------------------------------- named cases
# name -> (stakes, calls); a call is (blocks, register_only). Every case runs through both models
# (test_votes_model.py) and through the GPU against CellRule (test_gpu_votes.py).
def _voters(target, authors, rnd, s, e):
    return [block(a, rnd, [("range", target[1], s, e)], tag=("v", s, e)) for a in authors]


def named_cases():
    cases = {}
    eq4 = [1, 1, 1, 1]  # quorum 3

    # Shares at 0, 2, 3; votes at 1, 4 (for an unseen block); others vote [0, 5)
    other = ref_of(3, 77, "never")
    mixed = block(0, 1, [("share", b"a"), ("vote", other, 0), ("share", b"b"), ("share", b"c"), ("range", other, 0, 2)])
    cases["interleaved"] = (eq4, [([mixed] + _voters(mixed, [1, 2, 3], 2, 0, 5), False)])

    # 2S/3 + 1 crossed exactly: stakes 5 3 2 1 1 -> S = 12, quorum 9
    st = [5, 3, 2, 1, 1]
    b = block(1, 1, shares(2))  # stake 3
    cases["threshold_exact"] = (st, [([b] + _voters(b, [0], 2, 0, 1) + _voters(b, [3], 2, 0, 2), False),  # 0: 3 + 5 = 8, then + 1 = 9; 1: 4
                                     (_voters(b, [0], 3, 1, 2), False),  # 1: 9
                                     ])
    cases["threshold_one_less"] = (st, [([b] + _voters(b, [2, 3, 4], 2, 0, 2), False)])  # 7 < 9

    # a voter twice: within one block, across blocks of a call, across calls
    b = block(0, 1, shares(1))
    twice = block(1, 2, [("range", b[1], 0, 1), ("vote", b[1], 0), ("range", b[1], 0, 1)])
    cases["voter_twice"] = (eq4, [([b, twice, twice[:2] + (twice[2][:1],)], False), (_voters(b, [1], 3, 0, 1), False),
                                  (_voters(b, [2], 4, 0, 1) + _voters(b, [3], 4, 0, 1), False)])

    # one authority holds a quorum: registering does not certify, the next vote by anyone does
    big = [10, 1, 1]
    b = block(0, 1, shares(2))
    cases["single_quorum"] = (big, [([b], False), (_voters(b, [0], 2, 0, 1) + _voters(b, [2], 2, 1, 2), False)])

    # order inside one call: a vote ahead of the registration is unknown, the same vote after it
    # counts; the first block that crosses certifies; later votes are unknown
    b = block(0, 5, shares(3))
    early = _voters(b, [1], 4, 0, 3)
    # (nine equal stakes: quorum 7, crossed by the seventh voter; three blocks vote after it)
    cases["order_in_call"] = ([1] * 9, [(early + [b] + early + _voters(b, [2, 3, 4, 5, 6, 7, 8], 6, 0, 3) + early, False)])

    # VoteRange edges
    b = block(0, 1, shares(6))
    top = (1 << 20) - 1
    unseen = ref_of(2, 9, "unseen")
    e = block(1, 2, [("range", b[1], 2, 2), ("range", b[1], top, top), ("range", b[1], 4, 40), ("range", unseen, 0, top),
                     ("range", unseen, 5, top + 5), ("range", b[1], 0, top)])
    # one range over cells in three states: [0, 2) certified, [2, 4) aggregating, [6, 8) never registered
    three = (_voters(b, [2, 3], 3, 0, 2) + [block(4, 4, [("range", b[1], 0, 8)])])
    cases["range_edges"] = (eq4 + [1], [([b, e], False), (three, False)])

    # Vote edges: Accept as a one-cell range, both Reject forms and offset 2^64 - 1 flagged and ignored
    b = block(0, 1, shares(2))
    v = block(1, 2, [("vote", b[1], 1), ("reject", b[1], 0, None), ("reject", b[1], 0, (b[1], 1)), ("vote", b[1], U64),
                     ("range", b[1], 5, 3), ("vote", b[1], 0), ("vote", b[1], 7)])
    cases["vote_edges"] = (eq4, [([b, v], False), (_voters(b, [2], 3, 0, 2), False)])

    # the same block twice: duplicates, state unchanged; and again after it was certified
    b = block(0, 1, [("share", b"x"), ("vote", other, 3), ("share", b"y")])
    cases["block_twice"] = (eq4, [([b, b], False), ([b], False), (_voters(b, [1, 2], 2, 0, 1), False),
                                  ([b] + _voters(b, [1], 3, 0, 3) + [b] + _voters(b, [2, 3], 4, 0, 3), False)])

    # handle_proposal: register only (its votes are not looked at), then others certify
    own = block(0, 1, shares(2) + [("range", other, 0, 4), ("reject", other, 0, None)])
    cases["register_only"] = (eq4, [([own], True), (_voters(own, [1, 2], 2, 0, 2), False)])

    # many targets, wide ranges: 64 sharing blocks x 300 Shares, every authority votes [0, 300) on
    # every one, with ranges that split them at odd offsets first
    st7 = unequal_stakes(7)
    sharing = [block(k % 7, 1, shares(300), tag=k) for k in range(64)]
    votes = []
    for a in range(7):
        sts = []
        for k, b in enumerate(sharing):
            if (a + k) % 3 == 0:
                sts.append(("range", b[1], 1 + (k % 5), 67 + 2 * a + k))
            sts.append(("range", b[1], 0, 300))
            if k % 11 == a:
                sts.append(("range", b[1], 129 + a, 131 + a))
        votes.append(block(a, 2, sts, tag="wide"))
    cases["wide"] = (st7, [(sharing + votes, False)])
    return cases
