"""CPU: the plain-Python model of mv_encode_blocks (tests/encode_model.py) is pinned to the builder's
writer (mysticeti_amd/blocks.py: encode), to the C oracle's parse of what it wrote, and -- through
tests/seal_model.py -- to build_rounds_sealed's DAG; its refusals to the cases of
include/mysti_verify.h. No GPU."""
import numpy as np
import pytest

import encode_cases as C
import encode_model as EM
import oracle as O
import seal_model as S
from mysticeti_amd import blocks as BL


def spec_blocks(which):
    """[(author, round, includes, shares, ranges, time_ns, epoch)] of config-1 and config-4 shape."""
    if which == "config1":
        n_auth, n_inc, n_vr, tx = 4, 4, 0, False
    else:
        n_auth, n_inc, n_vr, tx = 100, 67, 66, True
    gen = BL.genesis_refs(n_auth)
    out = []
    for r in (1, 2):
        prev = gen if r == 1 else [(a, 1, C.digest("prev", a)) for a in range(n_auth)]
        for a in (0, 1, n_auth - 1):
            others = [x for x in range(n_auth) if x != a]
            inc = [prev[a]] + [prev[x] for x in others[:n_inc - 1]]
            shares = [BL.config4_tx(r, a)] if tx else []
            ranges = [(prev[(a + 1 + v) % n_auth], 0, 1 + v % 7) for v in range(n_vr)]
            out.append((a, r, inc, shares, ranges, ((r + 5) << 64) + r * 10**8 + a, 3))
    return out


@pytest.mark.parametrize("which", ["config1", "config4"])
def test_model_equals_the_builder_and_the_oracle_parses_it(which):
    c = C.Call(which)
    want = []
    for a, r, inc, shares, ranges, t, ep in spec_blocks(which):
        # the Shares and the VoteRanges as two payloads: their bodies under one count
        j0 = c.pay(EM.payload([("share", s) for s in shares]), align=len(want) % 8)
        c.pay(EM.payload([("range", ref, lo, hi) for ref, lo, hi in ranges]), align=(3 * len(want)) % 8)
        c.block(a, r, inc, j0, 2, time_ns=t, epoch=ep)
        want.append(BL.encode(a, r, inc, shares, ranges, t, ep, bytes(64), bytes(32)))
    res = c.model()
    assert res.status == [EM.OK] * len(want) and res.out_bytes == len(res.buf)
    for (bn, pre), o, l in zip(want, res.offs, res.lens):
        got = bytes(res.buf[o:o + l])
        assert got == bn
        assert o % 8 == 0 and not any(res.buf[o + l:(o + l + 7) & ~7])
        assert O.block_preimage(got) == pre  # the C oracle parses it and gives the same pre-image
        assert S.preimage(got) == pre


def test_lengths_and_layout():
    c = C.shapes()
    res = c.model()
    assert res.status == c.want == [EM.OK] * len(c.heads)
    pos = 0
    for h, o, l in zip(c.heads, res.offs, res.lens):
        bodies = sum(c.plen[j] - 8 for j in range(h[8], h[8] + h[9]))
        assert l == 169 + 56 * h[7] + bodies and o == pos
        pos += (l + 7) & ~7
        assert S.parse(bytes(res.buf[o:o + l])) is not None
    assert res.out_bytes == pos == len(res.buf)
    assert {l % 8 for l in res.lens} == set(range(8))  # every padding length occurs
    assert C.WG_BYTES - 1 in res.lens and C.WG_BYTES in res.lens


def test_refusals_take_no_space_and_leave_their_neighbours():
    c = C.refusals()
    res = c.model()
    assert res.status == c.want
    refused = {i for i, s in enumerate(res.status) if s != EM.OK}
    assert {res.status[i] for i in refused} == {EM.BAD_HEAD, EM.BAD_PAYLOAD} and len(refused) >= 60
    assert all(res.lens[i] == 0 and res.offs[i] == res.offs[i + 1] for i in refused)
    assert all(res.status[i - 1] == res.status[i + 1] == EM.OK for i in refused)
    less = c.without(refused).model()
    assert bytes(less.buf) == bytes(res.buf) and less.out_bytes == res.out_bytes
    assert less.offs == [o for i, o in enumerate(res.offs) if i not in refused]


def test_too_long_one_unit_either_side():
    c = C.too_long()
    res = c.model()
    assert res.status == c.want == [EM.OK, EM.TOO_LONG, EM.TOO_LONG, EM.BAD_HEAD, EM.OK]
    assert res.lens[0] == EM.MAX_LEN == 8388600 and res.lens[1:4] == [0, 0, 0]
    assert S.parse(bytes(res.buf[:res.lens[0]])) is not None


def test_cap_rule():
    c = C.refusals()
    full = c.model()
    out = bytearray(b"\xa5" * (full.out_bytes + 24))
    short = c.model(cap=full.out_bytes - 8, out=out)
    assert short.buf is None and out == b"\xa5" * len(out)
    assert (short.offs, short.lens, short.status, short.out_bytes) == (full.offs, full.lens, full.status, full.out_bytes)
    exact = c.model(cap=full.out_bytes, out=out)
    assert exact.buf is out and bytes(out[:full.out_bytes]) == bytes(full.buf) and out[full.out_bytes:] == b"\xa5" * 24


class ModelSigner:
    def ed25519_sign(self, seeds, msgs):
        return None, np.array([list(S.sign(bytes(s), bytes(m))) for s, m in zip(seeds, msgs)], dtype=np.uint8)


class ModelSealer:
    """Stands in for Engine in blocks.build_rounds_sealed: seal_blocks by the model."""

    def seal_blocks(self, buf, offs, lens, seeds, link=False):
        raw = bytearray(buf.tobytes())
        st, md, bd = S.seal(raw, [int(o) for o in offs], [int(l) for l in lens], [bytes(s) for s in seeds], link=link)
        buf[:] = np.frombuffer(bytes(raw), dtype=np.uint8)
        return np.array(st, dtype=np.uint8), md, bd


@pytest.mark.parametrize("n_auth,rounds,n_inc,n_vr,tx", [(4, 3, 4, 0, False), (5, 2, 4, 3, True)])
def test_sealed_linked_dag_equals_build_rounds_sealed(n_auth, rounds, n_inc, n_vr, tx):
    """blocks.encoded_inputs through the model, sealed and linked by seal_model, is
    build_rounds_sealed's DAG sealed by seal_model."""
    seeds = [BL.authority_seed(a) for a in range(n_auth)]
    want = BL.build_rounds_sealed(ModelSealer(), rounds, n_auth, seeds, n_inc, n_vr, tx)
    heads, includes, (pbuf, poff, plen) = BL.encoded_inputs(rounds, n_auth, n_inc, n_vr, tx)
    res = EM.encode(heads.tolist(), includes.tolist(), pbuf.tobytes(), poff.tolist(), plen.tolist())
    assert res.status == [EM.OK] * len(want)
    st, _, _ = S.seal(res.buf, res.offs, res.lens, seeds, link=True)
    assert st == [S.OK] * len(want)
    assert [bytes(res.buf[o:o + l]) for o, l in zip(res.offs, res.lens)] == want
    # config 1 without VoteRanges is build_rounds' DAG too
    if n_vr == 0:
        assert want == BL.build_rounds(ModelSigner(), rounds, n_auth, seeds, n_inc, n_vr, tx)


def test_the_library_exports_the_encode_calls():
    """In EXPORTS, defined in the shared library, declared in the header with the argument counts
    the ctypes mirror gives them; the constants agree in header, mirror and model."""
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
    for name, n_args in (("mv_encode_blocks", 22), ("mv_dev_encode_blocks", 24)):
        assert name in M.EXPORTS and name in defined, name
        fn = getattr(lib, name)
        assert isinstance(fn, ctypes._CFuncPtr) and len(fn.argtypes) == n_args, name
        decl = re.search(r"mv_status\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl and len(decl.group(1).split(",")) == n_args, name
    assert (M.ENCODE_OK, M.ENCODE_BAD_HEAD, M.ENCODE_BAD_PAYLOAD, M.ENCODE_TOO_LONG) == \
        (EM.OK, EM.BAD_HEAD, EM.BAD_PAYLOAD, EM.TOO_LONG) == (0, 1, 2, 3)
    assert M.ENCODE_STATUS == EM.STATUS and (M.ENCODE_SEAL, M.ENCODE_LINK) == (1, 2)
    assert M.ENCODE_MAX_LEN == EM.MAX_LEN and M.ENCODE_HEAD_WORDS == EM.HEAD_WORDS
    for code, value in (("MV_ENCODE_OK", 0), ("MV_ENCODE_BAD_HEAD", 1), ("MV_ENCODE_BAD_PAYLOAD", 2),
                        ("MV_ENCODE_TOO_LONG", 3), ("MV_ENCODE_SEAL", 1), ("MV_ENCODE_LINK", 2),
                        ("MV_ENCODE_MAX_LEN", EM.MAX_LEN)):
        assert re.search(r"#define\s+%s\s+%du?\b" % (code, value), header), code
    kernels = open(os.path.join(root, "mysticeti_amd", "csrc", "kernels.h")).read()
    assert re.search(r"EN_WG_BYTES = %d;" % C.WG_BYTES, kernels)  # the case lists straddle the kernels' switch
    assert re.search(r"EN_TILE = %d;" % C.TILE, kernels)
    for method in ("encode_blocks", "dev_encode_blocks"):
        assert callable(getattr(M.Engine, method)), method
    assert callable(BL.build_rounds_encoded)
