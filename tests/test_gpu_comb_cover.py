"""GPU: every kernel that sums comb-table entries, on inputs that reach every (row, digit) pair.

A valid signature is accepted only if each of its 64 looked-up entries, digits and signs is right,
so the covers of tests/comb_model.py -- b_cover for the B table (s's digit is j in every row, j =
-128..127, and 0..16 in row 31) and a_cover for a key's A table (k's digits take every value in
every row) -- make "status 0" a check of all 7,953 reachable pairs in whichever kernel verified
them; a control (s + 256^row) must come back with the oracle's status, so a kernel that accepts
everything fails too. tests/test_comb_model.py has shown both oracles accept every cover element
and reject every control. The consumers, each with its own digit decoding and row split:

  k_verify_comb     ct_sum, rows 0..31 (B) and 0..15 / 16..31 (A)           signature calls, MV_COMB_QUAD=0
  k_verify_comb16   q_ct_sum_pf, blocks of 8 rows (B) and 4 rows (A)        signature calls, MV_COMB_QUAD=1
  k_online          the same body per job, blocks ingested and hashed       block calls, 1 / 3 / 4 / 64 per call
  k_verify_comb16   with ingest and hashing inside                          block calls, online=False
  k_hash_comb_pre + k_comb_post   ct_sum over B; q_ct_sum, 8 roles of 4 rows  block calls, MV_COMB_SPLIT_BYTES=1
  k_bv_keycol       ct_sum over one row per lane, then a tree               Engine.batch_msm, per-key form
  k_bv_final        ct_sum(combB) of the reduced column sums                Engine.batch_msm

A failure names the consumer, the key, the digits (or the row a control moved) and the statuses."""
import functools

import numpy as np
import pytest

import comb_model as CM
import msm_model as MM
import mysticeti_amd as M
import mysticeti_amd.blocks as MB
import oracle as O
import zip215 as Z

pytestmark = pytest.mark.gpu


class Case:
    def __init__(self, kind, key, item, sig, row=None, block=None):
        self.kind, self.key, self.item, self.sig, self.row, self.block = kind, key, item, sig, row, block

    def __str__(self):
        what = f"control: s + 256^{self.row} of" if self.kind == "control" else "cover:"
        return (f"key {self.key} {what} s digits {list(self.item.s_digits)}, "
                f"k digits {list(self.item.k_digits) if self.item.k_digits else 'any (small-order key)'}")


def u8(rows):
    return np.array([np.frombuffer(r, np.uint8) for r in rows])


def set_committee(eng):
    com = CM.committee()
    ok = eng.set_committee(com.pks, com.stakes, 0)
    assert ok.all()
    return com


# ---------------------------------------------------------------- signature calls
@functools.lru_cache(maxsize=None)
def sig_cases():
    """(covers, controls): the B cover under the small-order key and the A covers of the first, a
    middle and the last key; one control per row and cover. Each carries the oracle's status."""
    com = CM.committee()
    covers, ctl = [], []
    for key, items in [(com.small, CM.b_cover())] + [(k, CM.key_cover(k)) for k in com.a_keys]:
        covers += [Case("cover", key, it, it.sig) for it in items]
        ctl += [Case("control", key, items[n], sig, row=i) for n, i, sig in CM.controls(items)]
    for cs, want in ((covers, 0), (ctl, 1)):
        st = O.verify_batch(com.pks[[c.key for c in cs]], u8([c.sig for c in cs]), u8([c.item.msg for c in cs]))
        assert (st == want).all()
        for c in cs:
            c.want = want
    return covers, ctl


def mixed(covers, ctl):
    out, step = [], len(covers) // len(ctl)
    for i, c in enumerate(covers):
        out.append(c)
        if i % step == step - 1 and i // step < len(ctl):
            out.append(ctl[i // step])
    assert len(out) == len(covers) + len(ctl)
    return out


@pytest.mark.parametrize("quad,kernel", [(0, "k_verify_comb"), (1, "k_verify_comb16")])
def test_signature_calls(engine, quad, kernel):
    set_committee(engine)
    covers, ctl = sig_cases()
    assert len(covers) == 258 + sum(len(CM.key_cover(k)) for k in CM.committee().a_keys)
    for key in (CM.committee().small,) + CM.committee().a_keys:  # what this consumer is about to be held to
        mine = [c.item for c in covers if c.key == key]
        assert len(CM.pairs_of(mine, "s" if key == CM.committee().small else "k")) == CM.PAIRS
    orders = {"covers first": covers + ctl, "covers last": ctl + covers, "mixed": mixed(covers, ctl)}
    for name, cases in orders.items():
        n = len(cases)
        assert n % 4 and n % 64 and n < M.BATCH_MIN  # a ragged tail workgroup; below the batch path
        with engine.option("MV_COMB_QUAD", quad):
            st = engine.ed25519_verify(u8([c.item.msg for c in cases]), u8([c.sig for c in cases]),
                                       key_idx=np.array([c.key for c in cases], np.uint32))
        bad = [f"{kernel} ({name}, position {i} of {n}): {c}: status {int(s)}, want {c.want}"
               for i, (c, s) in enumerate(zip(cases, st)) if int(s) != c.want]
        assert not bad, f"{len(bad)} wrong; first:\n" + "\n".join(bad[:5])


# ---------------------------------------------------------------- block calls
@functools.lru_cache(maxsize=None)
def block_cases():
    """(covers, controls) as whole blocks: the A cover of one key (the middle one), ground over the
    block's creation time, and the B cover under the small-order author. want = the C oracle's
    (status, message digest, block digest)."""
    com = CM.committee()
    key = com.a_keys[1]
    covers, ctl = [], []
    for author, blocks in ((key, CM.block_a_cover(key)), (com.small, CM.block_b_cover())):
        covers += [Case("cover", author, b.item, b.item.sig, block=b) for b in blocks]
        ctl += [Case("control", author, blocks[n].item, c.bincode[-64:], row=i, block=c)
                for n, i, c in CM.block_controls(blocks)]
    for cs, want in ((covers, 0), (ctl, 6)):
        for c in cs:
            c.want = O.block_verify(c.block.bincode, com.pks, com.stakes, 0)
            assert c.want == (want, c.block.msg_digest, c.block.digest)
    # the product's own encoder spells the same bytes
    c = covers[0]
    t = CM.block_template(c.key, c.item.cand)
    bn, pre = MB.encode(c.key, 2, [(r.authority, r.round, r.digest) for r in t.includes], [b"comb cover"], [],
                        t.meta_creation_time_ns, 0, c.sig, c.block.digest)
    assert bn == c.block.bincode and pre == t.preimage()
    return covers, ctl


def sub_block_cases():
    """The one-block-per-call subset: every pair of comb_model.sub_pairs() -- digits -128, -1, 0, 1,
    127 in rows 0, 7, 8, 15, 16, 23, 24, 30 and (0, 1 only) 31, the first and last row of every
    wave's and role's row block -- in the A cover and in the B cover, and the controls of those rows."""
    covers, ctl = block_cases()
    com = CM.committee()
    out = []
    for author, which in ((com.a_keys[1], "k"), (com.small, "s")):
        mine = [c for c in covers if c.key == author]
        keep = {id(it) for it in CM.sub_cover([c.item for c in mine], which)}
        sub = [c for c in mine if id(c.item) in keep]
        assert CM.sub_pairs() <= CM.pairs_of([c.item for c in sub], which)
        out += sub + [c for c in ctl if c.key == author and c.row in CM.SUB_ROWS]
    return out


def run_blocks(eng, consumer, cases, per_call):
    calls = 0
    bad = []
    for lo in range(0, len(cases), per_call):
        part = cases[lo:lo + per_call]
        st, md, bd = eng.verify_blocks([c.block.bincode for c in part])
        calls += 1
        for j, c in enumerate(part):
            got = (int(st[j]), md[j].tobytes(), bd[j].tobytes())
            if got != c.want:
                bad.append(f"{consumer} (block {lo + j}, {j} of its call): {c}: status {got[0]}, want {c.want[0]}; "
                           f"digests {'equal' if got[1:] == c.want[1:] else 'differ'}")
    assert not bad, f"{len(bad)} wrong; first:\n" + "\n".join(bad[:5])
    return calls


@pytest.mark.parametrize("per_call", [1, 3, 4, 64])
def test_online_service_blocks(engine, per_call):
    """k_online: 1 and 3 per call take the speculative R decode, 4 the parse-then-decode workgroup, 64
    sixteen jobs. One per call runs the stated subset, the others the full covers."""
    set_committee(engine)
    covers, ctl = block_cases()
    cases = sub_block_cases() if per_call == 1 else mixed(covers, ctl)
    o0 = engine.online_stats()[0]
    calls = run_blocks(engine, f"k_online, {per_call} per call", cases, per_call)
    assert engine.online_stats()[0] - o0 == calls  # the resident service took every call


def test_submission_queue_blocks():
    covers, ctl = block_cases()
    with M.Engine(devices=(0,), online=False) as eng:
        set_committee(eng)
        cases = mixed(covers, ctl)
        assert len(cases) % 4 and len(cases) < M.BATCH_MIN
        run_blocks(eng, "k_verify_comb16 with ingest (queue)", cases, len(cases))
        run_blocks(eng, "k_verify_comb16 with ingest (queue)", ctl + covers, len(cases))
        assert eng.online_stats()[0] == 0


def test_split_form_blocks(engine, opts):
    opts("MV_COMB_SPLIT_BYTES", 1)
    opts("MV_ONLINE", 0)
    set_committee(engine)
    covers, ctl = block_cases()
    cases = mixed(covers, ctl)
    run_blocks(engine, "k_hash_comb_pre + k_comb_post", cases, len(cases))
    run_blocks(engine, "k_hash_comb_pre + k_comb_post", ctl + covers, len(cases))


# ---------------------------------------------------------------- the batch path's two table sums
GROUPS = MM.MAX_GROUPS
# the fewest rows mv_selftest_batch_msm takes in 16 groups: it has no minimum of its own (engine.cpp
# refuses only n = 0 and scalars out of range), and a group is at least one 1024-signature chunk
N_MSM = (GROUPS - 1) * MM.GROUP_CHUNK + 1
B_ROW = np.array(MM.point_row(MM.affine(Z.B_POINT)), dtype=np.uint32)
W_ONE_B = [Z.B_POINT] + [Z.IDENTITY] * (MM.NWR - 1)  # z = 1 on R = B: window 0 holds B


def msm_call(engine, key, c, x):
    """One batch_msm call in the per-key form: group g has one live row (z = 1, R = B, z k = c[g],
    key `key`) and column sums spelling x[g]. Returns (BatchMsm, cols)."""
    assert len(c) == len(x) <= GROUPS
    n = N_MSM if len(c) == GROUPS else (len(c) - 1) * MM.GROUP_CHUNK + 1
    scal = np.zeros((n, 12), dtype=np.uint32)
    for g, cg in enumerate(c):
        scal[g * MM.GROUP_CHUNK] = MM.scalar_row(1, cg)
    cols = np.zeros((GROUPS, 12), dtype=np.uint64)
    for g, xg in enumerate(x):
        cols[g] = MM.columns_of(xg)
    out = engine.batch_msm(scal, np.tile(B_ROW, (n, 1)), cols, groups=GROUPS,
                           key_idx=np.full(n, key, np.uint32), n_keys=len(CM.committee().pks))
    assert (out.groups, out.group_sigs) == (len(c), MM.GROUP_CHUNK)
    return out, cols


def chunks(seq, k=GROUPS):
    return [seq[i:i + k] for i in range(0, len(seq), k)]


@pytest.mark.parametrize("key", CM.committee().a_keys)
def test_batch_per_key_term(engine, key):
    """k_bv_keycol: the column sum c_b of key b is exactly a B-cover scalar (one live row per group),
    16 groups per call: asum[g] must be [c]A_b, and with columns spelling 1 + c a_b the flag 1."""
    com = set_committee(engine)
    a = com.secrets[key]
    A = Z.decompress(com.pks[key].tobytes())
    scalars = CM.b_scalars()
    assert len(CM.pairs_of(CM.b_cover(), "s")) == CM.PAIRS
    for lo, c in zip(range(0, len(scalars), GROUPS), chunks(scalars)):
        out, cols = msm_call(engine, key, c, [(1 + cg * a) % Z.L for cg in c])
        for g, cg in enumerate(c):
            want = Z.scalarmult(A, cg)
            assert MM.equation_holds(W_ONE_B, cols[g], want)
            assert MM.row_equals(out.asum[g], want), \
                f"k_bv_keycol: key {key}, cover scalar {lo + g}, digits {CM.recode256(cg)}: asum is not [c]A"
            assert out.flags[g] == 1, f"k_bv_final after k_bv_keycol: key {key}, digits {CM.recode256(cg)}: flag 0"


def test_batch_final_b_term(engine):
    """k_bv_final's [bsum]B: the column sums spell a B-cover scalar x, and the per-key term is chosen
    so that B + [c]A = [x]B: every flag 1; with x + 256^row (one control per row) the flag the
    model's equation gives, 0."""
    com = set_committee(engine)
    key = com.a_keys[0]
    a = com.secrets[key]
    A = Z.decompress(com.pks[key].tobytes())
    ainv = pow(a, -1, Z.L)
    scalars = CM.b_scalars()
    ctl = [(n, i, (CM.sig_s(sig)) % Z.L) for n, i, sig in CM.controls(CM.b_cover())]
    jobs = [(f"cover scalar {n}", s, s) for n, s in enumerate(scalars)] + \
           [(f"control: cover scalar {n} + 256^{i}", scalars[n], x) for n, i, x in ctl]
    for part in chunks(jobs):
        c = [(s - 1) * ainv % Z.L for _, s, _ in part]
        out, cols = msm_call(engine, key, c, [x for _, _, x in part])
        for g, (what, s, x) in enumerate(part):
            asum = Z.scalarmult(A, c[g])
            want = int(MM.equation_holds(W_ONE_B, cols[g], asum))
            assert want == int(x == s)
            assert MM.row_equals(out.asum[g], asum), f"k_bv_keycol: {what}: asum"
            assert out.flags[g] == want, \
                f"k_bv_final [bsum]B: {what}, digits {CM.recode256(x)}: flag {out.flags[g]}, want {want}"
