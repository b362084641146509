"""CPU: the plain-Python model of mv_seal_blocks (tests/seal_model.py) is pinned to RFC 8032 7.1
and to the builder it must reproduce (mysticeti_amd/blocks.py: encode, the digest helper and
build_rounds), and its link rule to the cases of include/mysti_verify.h. No GPU, no library."""
import numpy as np
import pytest

import seal_cases as C
import seal_model as S
from mysticeti_amd import blocks as BL

M_STATUS = ["OK", "PARSE_ERROR", "UNKNOWN_AUTHOR", "UNLINKED"]

# RFC 8032 section 7.1, TEST 1-3: secret key, public key, message, signature
RFC8032 = [
    ("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
     "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
    ("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
     "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
    ("c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7",
     "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025", "af82",
     "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac"
     "18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"),
]


@pytest.mark.parametrize("sk,pk,msg,sig", RFC8032)
def test_rfc8032_vectors(sk, pk, msg, sig):
    seed = bytes.fromhex(sk)
    assert S.expand(seed)[2].hex() == pk
    assert S.sign(seed, bytes.fromhex(msg)).hex() == sig


class ModelSigner:
    """Stands in for Engine in blocks.build_rounds: one signing call per round, by the model."""

    def ed25519_sign(self, seeds, msgs):
        sig = np.array([list(S.sign(bytes(s), bytes(m))) for s, m in zip(seeds, msgs)], dtype=np.uint8)
        return None, sig


def small_dag(rounds=3, n_auth=5):
    """A config-4-shape DAG small enough for Python integers: Shares, VoteRanges, distinct seeds."""
    seeds = [BL.authority_seed(a) for a in range(n_auth)]
    return BL.build_rounds(ModelSigner(), rounds, n_auth, seeds, n_inc=4, n_vr=3, with_tx=True), seeds


def test_preimage_matches_encode():
    gen = BL.genesis_refs(4)
    cases = [
        (1, 1, gen, [], [], 7, 0),
        (2, 5, gen[:3], [b"", b"x" * 200], [(gen[0], 0, 3), (gen[1], 2, 9)], (5 << 64) + 12, 3),
        (0, 0, [], [], [], 0, 0),
    ]
    for a, r, inc, shares, ranges, t, ep in cases:
        bn, pre = BL.encode(a, r, inc, shares, ranges, t, ep, bytes(range(64)), bytes(range(32)))
        assert S.preimage(bn) == pre
        assert S.preimage(bn + b"trailing") == pre  # bincode allows trailing bytes
        assert S.preimage(bn[:-1]) is None
        assert S.b2(pre) == BL._b2(pre)
    assert [S.b2(S.preimage(BL.encode(a, 0, [], [], [], 0, 0, bytes(64), bytes(32))[0]) + bytes(64))
            for a in range(4)] == [g[2] for g in gen]


@pytest.mark.parametrize("which", ["config1", "small"])
def test_linked_seal_reproduces_the_builder(which):
    if which == "config1":
        blocks, seeds = BL.config1(ModelSigner(), 6), [bytes(32)] * 4
    else:
        blocks, seeds = small_dag()
    stripped = S.unseal(blocks)
    assert all(s != b for s, b in zip(stripped, blocks))
    buf, offs, lens = S.pack(stripped, gaps=[i % 8 for i in range(len(blocks))])
    want, _, _ = S.pack(blocks, gaps=[i % 8 for i in range(len(blocks))])
    st, md, bd = S.seal(buf, offs, lens, seeds, link=True)
    assert st == [S.OK] * len(blocks)
    assert buf == want
    assert bd == [b[24:56] for b in blocks]
    # without the link every block is sealed over the zeroed includes it was given: round 1 (whose
    # includes are genesis) still equals the builder, round 2 does not
    buf2, _, _ = S.pack(stripped)
    st2, _, bd2 = S.seal(buf2, *S.pack(stripped)[1:], seeds, link=False)
    n1 = len(seeds)
    assert st2 == [S.OK] * len(blocks) and bd2[:n1] == bd[:n1] and bd2[n1] != bd[n1]


def test_link_rule_cases():
    blocks, want_status, links = C.link_corpus()
    seeds = C.seeds()
    buf, offs, lens = S.pack(blocks, gaps=[3] * len(blocks))
    before = bytes(buf)
    st, md, bd = S.seal(buf, offs, lens, seeds, link=True)
    assert [M_STATUS[x] for x in st] == want_status
    for i, name in enumerate(want_status):
        cur = bytes(buf[offs[i]:offs[i] + lens[i]])
        if name != "OK":  # untouched, no digests
            assert cur == before[offs[i]:offs[i] + lens[i]] and md[i] == bd[i] == bytes(32)
            continue
        # digest over pre-image || signature, signature over the pre-image's digest
        pre, p = S.preimage(cur), S.parse(cur)
        sig = cur[p.sig_pos:p.sig_pos + 64]
        assert md[i] == S.b2(pre) and sig == S.sign(seeds[p.author], md[i]) and cur[24:56] == bd[i] == S.b2(pre + sig)
        if i in links:
            got = [cur[at:at + 32] for _, _, at in p.includes]
            assert got == [x if isinstance(x, bytes) else bd[x] for x in links[i]]
    # the guard bytes between and after the blocks
    mask = bytearray(len(buf))
    for o, l in zip(offs, lens):
        mask[o:o + l] = b"\x01" * l
    assert all(buf[k] == 0xA5 for k in range(len(buf)) if not mask[k])
    # rounds out of order: refused, nothing written; a parse error between them does not count
    swapped = [blocks[7], blocks[4], blocks[0]]
    buf, offs, lens = S.pack(swapped)
    before = bytes(buf)
    with pytest.raises(S.InvalidArg):
        S.seal(buf, offs, lens, seeds, link=True)
    assert bytes(buf) == before
    assert S.seal(buf, offs, lens, seeds, link=False)[0] == [S.OK, S.PARSE_ERROR, S.OK]
    # n = 0 and n = 1
    assert S.seal(bytearray(b"guard"), [], [], seeds, link=True) == ([], [], [])
    one = bytearray(blocks[0])
    assert S.seal(one, [0], [len(one)], seeds, link=True)[0] == [S.OK] and bytes(one) != blocks[0]


def test_include_count_past_the_length():
    b = C.blk(0, 1, [BL.genesis_refs(1)[0]])
    assert S.parse(b) is not None
    assert S.parse(C.overcount(b, 2**40)) is None
    assert S.parse(C.overcount(b, 2)) is None  # two claimed, one present: the second runs into the statements


def test_the_library_exports_the_seal_calls():
    """The ABI check of tests/test_abi.py for the two new entries: in EXPORTS, defined in the shared
    library, declared in the header with the argument counts the ctypes mirror gives them."""
    import ctypes
    import os
    import re
    import subprocess

    import mysticeti_amd as M

    lib = M.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\bT (mv_[a-z0-9_]+)", nm))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mysti_verify.h")).read(), flags=re.S)
    for name, n_args in (("mv_seal_blocks", 11), ("mv_dev_seal_blocks", 14)):
        assert name in M.EXPORTS and name in defined, name
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and len(fn.argtypes) == n_args, name
        decl = re.search(r"mv_status\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    assert (M.SEAL_OK, M.SEAL_PARSE_ERROR, M.SEAL_UNKNOWN_AUTHOR, M.SEAL_UNLINKED) == \
        (S.OK, S.PARSE_ERROR, S.UNKNOWN_AUTHOR, S.UNLINKED) == (0, 1, 2, 3)
    assert M.SEAL_STATUS == M_STATUS and M.SEAL_LINK == 1
    for code, value in (("MV_SEAL_OK", 0), ("MV_SEAL_PARSE_ERROR", 1), ("MV_SEAL_UNKNOWN_AUTHOR", 2),
                        ("MV_SEAL_UNLINKED", 3), ("MV_SEAL_LINK", 1)):
        assert re.search(r"#define\s+%s\s+%du?\b" % (code, value), header), code
    for method in ("seal_blocks", "dev_seal_blocks"):
        assert callable(getattr(M.Engine, method)), method
    assert callable(BL.build_rounds_sealed)
