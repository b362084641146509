"""GPU: the index of block references (mv_index_*) and the accept call (mv_accept_blocks,
mv_dev_accept_blocks, mv_dev_index_insert) against tests/index_model.py: TwoState restates
include/mysti_verify.h over a dict (and tests/test_index_model.py holds it to BlockManager's own
structures), RefTable gives the probe-length yardstick. Verdicts are the CPU oracle's. Every case
is compared with the model, never with another device form."""
import ctypes
import hashlib
import random
import struct

import numpy as np
import pytest

import index_model as IM
import mysticeti_amd as M
import replay_model as RM
import wal as W
from mysticeti_amd import blocks as MB

pytestmark = pytest.mark.gpu

N_AUTH, ROUNDS = 4, 12
S64 = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def corpus(engine):
    """48 signed config-1 blocks (12 rounds of 4, about 233 B each, four includes), the committee,
    the genesis references and the oracle's verdict function."""
    bins = MB.config1(engine, ROUNDS)
    pks, stakes = MB.committee(engine, N_AUTH, distinct=False)
    genesis = MB.genesis_refs(N_AUTH)
    verdicts = RM.oracle_verdicts(pks, stakes, 0)
    assert len(bins) == 48 and IM.run_verdicts(verdicts, bins) == [0] * 48
    return bins, (pks, stakes, 0), genesis, verdicts


@pytest.fixture(params=[64, 2], ids=["tag64", "tag2"])
def eng(request, engine, corpus, opts):
    """The session engine with the committee set, the tag width of the case and an empty index."""
    engine.set_committee(*corpus[1])
    opts("MV_INDEX_TAG_BITS", request.param)
    engine.index_clear()
    yield engine
    engine.index_clear()


@pytest.fixture
def eng64(engine, corpus):
    engine.set_committee(*corpus[1])
    engine.index_clear()
    return engine


def bad_signature(block: bytes) -> bytes:
    """One bit of the signature's s flipped and the digest recomputed over the new signature:
    parses, digest matches, signature invalid."""
    sig = bytearray(block[-64:])
    sig[40] ^= 0x10
    dig = hashlib.blake2b(M.block_preimage(block) + bytes(sig), digest_size=32).digest()
    return block[:24] + dig + block[56:-64] + bytes(sig)


def rand_refs(rng, n):
    return [(rng.randrange(N_AUTH), rng.randrange(1, 1 << 20), rng.randbytes(32)) for _ in range(n)]


def check_index(e, two, what=""):
    """Every reference the model knows has its state, and the counts and the WANTED list agree."""
    refs = list(two.state)
    if refs:
        got = e.index_lookup(refs).tolist()
        assert got == [two.state[r] for r in refs], what
    st = e.index_stats()
    assert (st.have, st.wanted) == two.counts(), (what, st.have, st.wanted, two.counts())
    assert st.have + st.wanted <= st.capacity
    rows, total = e.index_wanted()
    assert total == st.wanted and {IM.words_ref(r) for r in rows} == two.wanted(), what


def accept(e, two, blocks, groups=None, what=""):
    got = e.accept_blocks(blocks, groups)
    want = two.accept(blocks, groups)
    assert got.blk_status.tolist() == want.blk_status, (what, got.blk_status.tolist(), want.blk_status)
    assert got.blk_state.tolist() == want.blk_state, (what, got.blk_state.tolist(), want.blk_state)
    assert got.n_missing == want.n_missing, (what, got.n_missing, want.n_missing)
    assert np.array_equal(got.missing, IM.ref_words(want.missing)), what  # the same order
    return got, want


def model(corpus, e, seed_genesis=True):
    two = IM.TwoState(corpus[3], corpus[2] if seed_genesis else ())
    if seed_genesis:
        assert e.index_insert(corpus[2], M.REF_HAVE).tolist() == [0] * N_AUTH
    return two


# ---------------------------------------------------------------- insert / lookup
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_insert_lookup(eng, n):
    rng = random.Random(n)
    two = IM.TwoState(None)
    refs = rand_refs(rng, n)
    states = [rng.choice([M.REF_WANTED, M.REF_HAVE]) for _ in refs]
    for st in (M.REF_WANTED, M.REF_HAVE):
        part = [r for r, s in zip(refs, states) if s == st]
        if part:
            assert eng.index_insert(part, st).tolist() == two.insert(part, st)
    others = rand_refs(rng, 50)
    assert eng.index_lookup(others).tolist() == [0] * 50
    check_index(eng, two, n)
    print(f"n {n}: {vars(eng.index_stats())}")


@pytest.mark.parametrize("copies", [64, 1000])
def test_the_same_reference_many_times_in_one_call(eng, copies):
    """One wave, and several workgroups: one entry, and every prior is the state before the call."""
    rng = random.Random(copies)
    two = IM.TwoState(None)
    r, other = rand_refs(rng, 2)
    refs = [r] * copies + [other] + [r] * 3
    assert eng.index_insert(refs, M.REF_WANTED).tolist() == two.insert(refs, M.REF_WANTED) == [0] * len(refs)
    check_index(eng, two)
    assert eng.index_insert(refs, M.REF_HAVE).tolist() == two.insert(refs, M.REF_HAVE) == [1] * len(refs)
    check_index(eng, two)
    assert eng.index_insert(refs, M.REF_HAVE).tolist() == [2] * len(refs)
    st = eng.index_stats()
    assert (st.have, st.wanted) == (2, 0)


def test_raises(eng):
    rng = random.Random(7)
    a, b = rand_refs(rng, 2)
    assert eng.index_insert([a], M.REF_WANTED).tolist() == [M.REF_ABSENT]
    assert eng.index_insert([a], M.REF_HAVE).tolist() == [M.REF_WANTED]  # WANTED then HAVE raises
    assert eng.index_insert([b], M.REF_HAVE).tolist() == [M.REF_ABSENT]
    assert eng.index_insert([b], M.REF_WANTED).tolist() == [M.REF_HAVE]  # HAVE then WANTED stays HAVE
    assert eng.index_lookup([a, b]).tolist() == [M.REF_HAVE, M.REF_HAVE]
    st = eng.index_stats()
    assert (st.have, st.wanted) == (2, 0)
    with pytest.raises(M.MvError, match=r"\(-1\)"):
        eng.index_insert([a], 3)


def test_one_bit_neighbours_are_absent(eng):
    base = np.array([[3, 77, 0x1111111111111111, 0x2222222222222222, 0x3333333333333333, 0x4444444444444444]], dtype=np.uint64)
    assert eng.index_insert(base, M.REF_HAVE).tolist() == [0]
    near = []
    for word in range(6):  # the authority, the round, each of the four digest words
        for bit in (0, 31, 32, 63):
            r = base[0].copy()
            r[word] ^= np.uint64(1 << bit)
            near.append(r)
    near = np.array(near, dtype=np.uint64)
    assert eng.index_lookup(near).tolist() == [0] * len(near)
    assert eng.index_lookup(base).tolist() == [M.REF_HAVE]


def test_forced_tag_collisions_take_more_rounds(engine, corpus, opts):
    """With 2-bit tags most probes meet a foreign slot with their own tag: results as at 64 bits."""
    engine.set_committee(*corpus[1])
    rng = random.Random(11)
    refs = rand_refs(rng, 3000)
    out = {}
    for bits in (64, 2):
        opts("MV_INDEX_TAG_BITS", bits)
        engine.index_clear()
        prior1 = engine.index_insert(refs[:2000] + refs[:500], M.REF_WANTED).tolist()
        prior2 = engine.index_insert(refs[1000:], M.REF_HAVE).tolist()
        out[bits] = (prior1, prior2, engine.index_lookup(refs).tolist(), engine.index_stats().have, engine.index_stats().wanted)
    engine.index_clear()
    assert out[2] == out[64] and out[64][3:] == (2000, 1000)


# ---------------------------------------------------------------- growth
def test_growth_keeps_every_entry(engine):
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(8)
        assert vars(e.index_stats()) == dict(have=0, wanted=0, capacity=8, rebuilds=0, longest_probe=0)
        rng = random.Random(5)
        two = IM.TwoState(None)
        sizes = [1, 2, 5, 8, 17, 64, 100, 333, 566, 1000, 1000, 1000]
        assert sum(sizes) == 4096
        rebuilds = 0
        for k, n in enumerate(sizes):
            refs = rand_refs(rng, n)
            st = M.REF_HAVE if k % 3 else M.REF_WANTED
            assert e.index_insert(refs, st).tolist() == two.insert(refs, st)
            check_index(e, two, k)  # every earlier entry, with its state, after each rebuild
            s = e.index_stats()
            assert s.rebuilds >= rebuilds and s.capacity >= len(two.state)
            rebuilds = s.rebuilds
        print(f"growth: {vars(e.index_stats())}")
        assert rebuilds >= 5 and e.index_stats().capacity >= 4096
        cap = e.index_stats().capacity
        e.index_reserve(100)  # never shrinks
        assert e.index_stats().capacity == cap
        e.index_clear()
        assert vars(e.index_stats()) == dict(have=0, wanted=0, capacity=cap, rebuilds=rebuilds, longest_probe=0)
        assert e.index_lookup(list(two.state)[:100]).tolist() == [0] * 100
    finally:
        e.close()


def test_wanted_list_of_a_large_table(engine):
    """A table of 2^19 slots is 2048 workgroups of the WANTED count: each lane of the scan's one
    workgroup sums two of them (tables up to 2^18 slots give a lane one at most). 257 and 513
    WANTED entries lie scattered over all of them, with HAVE entries in between that are not listed."""
    e = M.Engine(devices=(0,))
    try:
        e.index_reserve(1 << 18)
        assert e.index_stats().capacity == 1 << 18
        for n in (257, 513):
            rng = random.Random(n)
            two = IM.TwoState(None)
            for refs, st in ((rand_refs(rng, n), M.REF_WANTED), (rand_refs(rng, 300), M.REF_HAVE)):
                assert e.index_insert(refs, st).tolist() == two.insert(refs, st)
            assert two.counts()[1] == n
            check_index(e, two, n)  # the listed set is the model's, and its count is n
            e.index_clear()
        assert e.index_stats().capacity == 1 << 18 and e.index_stats().rebuilds == 0
    finally:
        e.close()


# ---------------------------------------------------------------- attacker-shaped keys
def test_keys_that_differ_in_one_byte(eng64):
    """48 x 255 references that differ from one base in a single byte, every position and value: a
    probe start that ignored a byte position would chain 255 long."""
    base = bytes(range(100, 148))
    keys = []
    for pos in range(48):
        for x in range(1, 256):
            k = bytearray(base)
            k[pos] ^= x
            keys.append(bytes(k))
    words = np.frombuffer(b"".join(keys), dtype="<u8").reshape(-1, 6).copy()
    eng64.index_reserve(len(keys))
    eng64.index_clear()
    assert eng64.index_insert(words, M.REF_HAVE).tolist() == [0] * len(keys)
    assert eng64.index_lookup(words).tolist() == [M.REF_HAVE] * len(keys)
    st = eng64.index_stats()
    ref = IM.RefTable(2 * st.capacity)
    for k in keys:
        ref.insert(k)
    print(f"one-byte neighbours: {len(keys)} keys, capacity {st.capacity}, longest probe {st.longest_probe}, "
          f"reference table {ref.longest}")
    assert st.have == len(keys) and 1 <= st.longest_probe <= 4 * ref.longest


# ---------------------------------------------------------------- accept against the model
def test_accept_the_dag_in_one_call(eng, corpus):
    bins = corpus[0]
    two = model(corpus, eng)
    got, _ = accept(eng, two, bins, [0] * 48, "one call")
    assert got.blk_state.tolist() == [M.ACC_NEW] * 48 and got.n_missing == 0
    check_index(eng, two)
    got, _ = accept(eng, two, bins, None, "again")
    assert got.blk_state.tolist() == [M.ACC_KNOWN] * 48


def test_accept_round_by_round_in_reverse(eng, corpus):
    """Every include is missing once and only once across calls, WANTED shrinks as blocks arrive,
    and it ends empty."""
    bins = corpus[0]
    two = model(corpus, eng)
    seen = []
    for r in range(ROUNDS - 1, -1, -1):
        got, want = accept(eng, two, bins[4 * r:4 * r + 4], [r] * 4, f"round {r + 1}")
        seen += want.missing
        check_index(eng, two, r)
        assert eng.index_stats().wanted == (4 if r else 0)
    assert len(seen) == len(set(seen)) == 44  # rounds 1..11, once each; round 1 includes the genesis blocks


@pytest.mark.parametrize("seed", range(20))
def test_accept_random_orders(eng, corpus, seed):
    bins = corpus[0]
    rng = random.Random(seed)
    two = model(corpus, eng)
    order = list(range(48))
    rng.shuffle(order)
    order += rng.sample(order, 8)
    p = 0
    while p < len(order):
        m = rng.randint(1, 12)
        blocks = [bins[i] for i in order[p:p + m]]
        groups = None if rng.random() < 0.3 else sorted(rng.randrange(3) for _ in blocks)
        accept(eng, two, blocks, groups, (seed, p))
        p += m
    check_index(eng, two, seed)
    assert two.wanted() == set()


# ---------------------------------------------------------------- groups
def test_groups(eng, corpus):
    bins = corpus[0]
    two = model(corpus, eng)
    # a group with one flipped signature bit: its other blocks are DROPPED, nothing of it is
    # inserted and none of its includes is listed (they would be: round 2 comes before round 1)
    blocks = [bins[4], bad_signature(bins[5]), bins[6]]
    got, _ = accept(eng, two, blocks, [9, 9, 9], "rejected group")
    assert got.blk_state.tolist() == [M.ACC_DROPPED, M.ACC_REJECTED, M.ACC_DROPPED] and got.n_missing == 0
    assert got.blk_status.tolist() == [0, M.BLOCK_SIG_INVALID, 0]
    check_index(eng, two)
    assert eng.index_stats().have == N_AUTH and eng.index_stats().wanted == 0
    # a KNOWN block with a tampered body inside an otherwise good group
    accept(eng, two, [bins[0]], None, "first")
    tampered = bins[0][:100] + bytes([bins[0][100] ^ 0xFF]) + bins[0][101:]
    got, _ = accept(eng, two, [bins[1], tampered, bins[2]], [4, 4, 4], "tampered known block")
    assert got.blk_state.tolist() == [M.ACC_NEW, M.ACC_KNOWN, M.ACC_NEW] and got.blk_status.tolist() == [0, 0, 0]
    # the same block in three groups: the lowest accepted index is NEW, the rest DUP
    got, _ = accept(eng, two, [bins[3], bins[3], bins[3]], [1, 2, 3], "three groups")
    assert got.blk_state.tolist() == [M.ACC_NEW, M.ACC_DUP, M.ACC_DUP]
    # ... and with the first group rejected by another block, the second is NEW
    got, _ = accept(eng, two, [bins[8], bad_signature(bins[9]), bins[8], bins[8]], [1, 1, 2, 3], "first group rejected")
    assert got.blk_state.tolist() == [M.ACC_DROPPED, M.ACC_REJECTED, M.ACC_NEW, M.ACC_DUP]
    check_index(eng, two)


# ---------------------------------------------------------------- short and malformed references
def test_short_and_malformed_references(eng, corpus):
    bins = corpus[0]
    two = model(corpus, eng)
    accept(eng, two, [bins[0]], None, "a known block")
    word = lambda v: bins[0][:16] + struct.pack("<Q", v) + bins[0][24:]
    cases = [b"", bins[0][:1], bins[0][:55], bins[1][:56], word(31), word(33)]
    got, _ = accept(eng, two, cases + [bins[2]], None, "short")
    assert got.blk_state.tolist() == [M.ACC_REJECTED] * 6 + [M.ACC_NEW]
    assert got.blk_status.tolist() == [M.BLOCK_PARSE_ERROR] * 6 + [0]
    got, _ = accept(eng, two, cases, [0] * 6, "short, one group")
    assert got.blk_state.tolist() == [M.ACC_REJECTED] * 6
    check_index(eng, two)


def dev_accept(e, blocks, groups, cap, pad=16):
    """mv_dev_accept_blocks on a device buffer that ends `pad` bytes after the last block."""
    import torch

    dev = torch.device("cuda", 0)
    buf, offs, lens = MB.pack(blocks)
    total = int(lens.sum())
    d_buf = torch.zeros(total + pad, dtype=torch.uint8, device=dev)
    if total:
        d_buf[:total] = torch.from_numpy(buf[:total].copy()).to(dev)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)
    n = len(blocks)
    d_st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=dev)
    d_state = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=dev)
    d_miss = torch.full((cap + 2, 6), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    nm = e.dev_accept_blocks(0, d_buf, total, t64(offs), t64(lens), t64(groups) if groups is not None else None,
                             d_st[:n], d_state[:n], d_miss[:cap] if cap else None)
    st, state, miss = d_st.cpu().numpy(), d_state.cpu().numpy(), d_miss.cpu().numpy()
    w = min(nm, cap)
    assert (st[n:] == 0xAB).all() and (state[n:] == 0xAB).all() and (miss[w:] == -3).all()
    return M.Accepted(st[:n], state[:n], miss[:w].view(np.uint64), nm)


def test_device_call_with_a_short_block_last(eng, corpus):
    """The last block of the buffer is 55 bytes long and exactly 16 bytes of padding follow it."""
    bins = corpus[0]
    two = model(corpus, eng)
    eng.index_reserve(64)
    blocks = [bins[4], bins[5], bins[0][:55]]
    got = dev_accept(eng, blocks, [0, 0, 1], cap=16)
    want = two.accept(blocks, [0, 0, 1])
    assert got.blk_state.tolist() == want.blk_state == [M.ACC_NEW, M.ACC_NEW, M.ACC_REJECTED]
    assert got.blk_status.tolist() == want.blk_status and want.blk_status[2] == M.BLOCK_PARSE_ERROR
    assert got.n_missing == 4 and np.array_equal(got.missing, IM.ref_words(want.missing))
    check_index(eng, two)


# ---------------------------------------------------------------- caps
def test_caps(eng, corpus):
    bins = corpus[0]
    blocks = bins[8:12] + bins[16:20]  # rounds 3 and 5: eight includes missing
    total = 8
    for cap in (0, 1, total - 1, total, total + 3):
        eng.index_clear()
        two = model(corpus, eng)
        want = two.accept(blocks, None)
        assert want.n_missing == total
        buf, offs, lens = MB.pack(blocks)
        out = np.full((cap + 2, 6), S64, dtype=np.uint64)
        got = eng.accept_blocks_packed(buf, offs, lens, None, cap_missing=cap, missing_out=out)
        w = min(cap, total)
        assert got.n_missing == total and (out[w:] == S64).all(), cap
        assert np.array_equal(out[:w], IM.ref_words(want.missing)[:w]), cap
        check_index(eng, two, cap)
        # mv_index_wanted likewise
        out = np.full((cap + 2, 6), S64, dtype=np.uint64)
        n = ctypes.c_uint64(S64)
        rc = eng.lib.mv_index_wanted(eng.ctx, M._p(out) if cap else None, cap, ctypes.byref(n))
        assert rc == M.MV_OK and n.value == total and (out[w:] == S64).all(), cap
        assert {IM.words_ref(r) for r in out[:w]} <= two.wanted() and len({IM.words_ref(r) for r in out[:w]}) == w


# ---------------------------------------------------------------- batch size
def test_batch_size_call(eng64, corpus):
    """4,200 blocks in one call, 100 of them KNOWN and one with a bad signature: the 4,100 others
    take the walk and one combined equation. (mv_batch_counters counts batches and equations, not
    items: that exactly 4,100 blocks were verified shows in the 100 KNOWN states, which the call
    writes without a verdict, and in the batch path being taken at all, 4,100 >= MV_BATCH_MIN.)"""
    bins = corpus[0]
    two = model(corpus, eng64)
    assert eng64.index_insert([IM.own_ref(bins[0])], M.REF_HAVE).tolist() == two.insert([IM.own_ref(bins[0])], IM.HAVE)
    blocks = [bins[0] if i % 42 == 0 else bins[1 + i % 47] for i in range(4200)]
    blocks[2345] = bad_signature(blocks[2345])
    groups = [i // 100 for i in range(4200)]
    before = eng64.batch_counters()[0]
    got, want = accept(eng64, two, blocks, groups, "batch")
    print(f"batch: batches {before} -> {eng64.batch_counters()[0]}, states {np.bincount(got.blk_state, minlength=5).tolist()}")
    assert eng64.batch_counters()[0] == before + 1
    counts = np.bincount(got.blk_state, minlength=5).tolist()
    assert counts[M.ACC_KNOWN] == 100 and counts[M.ACC_REJECTED] == 1 and counts[M.ACC_DROPPED] > 0
    assert 4200 - 100 >= M.BATCH_MIN
    check_index(eng64, two)


# ---------------------------------------------------------------- device calls and the replay hand-off
def test_replay_hand_off(eng64, corpus):
    import torch

    bins = corpus[0]
    dev = torch.device("cuda", 0)
    w = W.WalWriter(12)
    for k in range(20):
        w.write(2, b"y" * (k % 8))
        w.write(3 if k % 4 == 1 else 1, (struct.pack("<Q", k) if k % 4 == 1 else b"") + bins[k])
    img = np.frombuffer(w.image(), dtype=np.uint8)
    d_img = torch.zeros(img.size + 64, dtype=torch.uint8, device=dev)
    d_img[:img.size] = torch.from_numpy(img.copy()).to(dev)
    cap = img.size // 16 + 1
    o = dict(d_pos=torch.zeros(cap, dtype=torch.int64, device=dev), d_tag=torch.zeros(cap, dtype=torch.int32, device=dev),
             d_len=torch.zeros(cap, dtype=torch.int32, device=dev), d_status=torch.zeros(cap, dtype=torch.uint8, device=dev),
             d_rows=torch.zeros((32, 10), dtype=torch.int64, device=dev),
             d_blk_status=torch.zeros(32, dtype=torch.uint8, device=dev),
             d_summary=torch.zeros(3, dtype=torch.int64, device=dev),
             d_last_seen=torch.zeros(N_AUTH, dtype=torch.int64, device=dev))
    torch.cuda.synchronize(dev)
    _, b = eng64.dev_wal_replay(0, d_img, img.size, w.pos, 12, **o)
    assert b == 20
    eng64.index_reserve(256)
    eng64.dev_index_insert(0, o["d_rows"], 10, b, M.REF_HAVE, word_offset=3)  # straight from HBM
    rows = o["d_rows"].cpu().numpy().view(np.uint64)[:b]
    two = IM.TwoState(corpus[3])
    two.insert([IM.own_ref(x) for x in bins[:20]], IM.HAVE)
    assert eng64.index_lookup(np.ascontiguousarray(rows[:, 3:9])).tolist() == [M.REF_HAVE] * b  # every row
    check_index(eng64, two)
    blocks = bins[20:24]  # the next round: all its includes were replayed
    got = dev_accept(eng64, blocks, [0] * 4, cap=8, pad=64)
    want = two.accept(blocks, [0] * 4)
    assert got.blk_state.tolist() == want.blk_state == [M.ACC_NEW] * 4 and got.n_missing == want.n_missing == 0
    check_index(eng64, two)


def test_index_full(engine, corpus):
    """The device calls cannot grow the index: MV_E_INDEX_FULL, and the index is unchanged."""
    import torch

    bins = corpus[0]
    dev = torch.device("cuda", 0)
    e = M.Engine(devices=(0,))
    try:
        e.set_committee(*corpus[1])
        two = IM.TwoState(corpus[3])
        refs = [IM.own_ref(b) for b in bins[:6]]
        # nothing reserved: nothing fits
        d_words = torch.from_numpy(IM.ref_words([IM.own_ref(b) for b in bins]).view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        with pytest.raises(M.MvError) as err:
            e.dev_index_insert(0, d_words, 6, 4)
        assert err.value.code == M.E_INDEX_FULL
        e.index_reserve(8)
        assert e.index_insert(refs, M.REF_HAVE).tolist() == two.insert(refs, IM.HAVE)
        probe = [IM.own_ref(b) for b in bins]
        before = e.index_lookup(probe).tolist()
        assert e.index_stats().capacity == 8
        with pytest.raises(M.MvError) as err:
            e.dev_index_insert(0, d_words, 6, 48)  # 6 + 48 > 8
        assert err.value.code == M.E_INDEX_FULL
        with pytest.raises(M.MvError) as err:
            dev_accept(e, bins[8:12], None, cap=4)  # 4 blocks + 16 includes
        assert err.value.code == M.E_INDEX_FULL
        assert e.index_lookup(probe).tolist() == before
        check_index(e, two)
        # what may fit goes in: the references of bins[6] and bins[7]
        e.dev_index_insert(0, d_words, 6, 2, word_offset=36)
        torch.cuda.synchronize(dev)
        two.insert([IM.own_ref(b) for b in bins[6:8]], IM.HAVE)
        check_index(e, two)
        assert e.index_stats().capacity == 8
    finally:
        e.close()


# ---------------------------------------------------------------- resources
def test_resources_return_after_destroy(engine, corpus):
    bins = corpus[0]
    base = engine.get_option("MV_LIVE_RESOURCES")
    e = M.Engine(devices=(0,))
    fresh = engine.get_option("MV_LIVE_RESOURCES")
    try:
        e.set_committee(*corpus[1])
        with_committee = engine.get_option("MV_LIVE_RESOURCES")
        assert e.index_lookup([IM.own_ref(bins[0])]).tolist() == [0]  # no index yet: nothing is made
        assert vars(e.index_stats())["capacity"] == 0 and e.index_wanted()[1] == 0
        e.index_clear()
        assert engine.get_option("MV_LIVE_RESOURCES") == with_committee
        e.index_reserve(8)
        e.index_insert(rand_refs(random.Random(1), 500), M.REF_WANTED)  # grows
        assert e.accept_blocks(bins[:8], [0] * 8).blk_state.tolist() == [M.ACC_NEW] * 8
        assert e.index_stats().rebuilds >= 1 and engine.get_option("MV_LIVE_RESOURCES") > with_committee
    finally:
        e.close()
    print(f"live resources: {base} -> {fresh} (fresh context) -> {engine.get_option('MV_LIVE_RESOURCES')}")
    assert engine.get_option("MV_LIVE_RESOURCES") == base
    e = M.Engine(devices=(0,))
    try:
        assert engine.get_option("MV_LIVE_RESOURCES") == fresh  # a fresh context holds what it held
    finally:
        e.close()
