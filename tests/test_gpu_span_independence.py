"""GPU: a block's verdict and digests depend on the bytes of its span alone.

The truncation tests put the next case's prefix or zeros behind a cut block, never the bytes the cut
block itself goes on with: a walker whose bound is a few bytes off would read exactly the bytes that
make the block parse. Here every block is followed by a 16-byte gap of zeros, of 0xFF, or of its own
continuation (for a whole block: the first bytes of a valid block), the block starts cycle through
the alignments 0..7, and every entry point that walks block bytes runs over each packing. Each
result is compared with the C oracle's StatementBlock::verify of the span's bytes alone (votes: with
votes_model.CellRule over the statements the test's own reader finds in them), never with another
fill's result. No buffer here ends where its data ends: reads outside a span are looked for on the
host (tests/test_walk_sanitized.py)."""
import numpy as np
import pytest

import blocks as B
import frames_model as FM
import mysticeti_amd as M
import oracle as O
from votes_model import CellRule
from walk_cases import count_attacks, decode_block, every_kind_block, small_committee

pytestmark = pytest.mark.gpu

GAP = 16
FILLS = ("zeros", "ones", "continuation")


def cases():
    """[(name, bytes, continuation)]: the cut blocks, the count attacks, 30 valid blocks."""
    whole, n_inc = every_kind_block()
    zeros = bytes(64)
    out = []
    # a statement's header: its u32 tag and the word after it (a Share's length, a locator's authority)
    cuts, pos = set(range(len(whole) - 140, len(whole))), 64 + 56 * n_inc + 8
    for st in decode_block(whole)[1]:
        cuts |= set(range(pos, pos + 12))
        pos += len(B.statement_bincode(_oracle_form(st)))
    assert pos == len(whole) - 25 - 8 - 64
    for k in sorted(cuts):
        out.append((f"cut at {k}", whole[:k], (whole[k:] + zeros)[:64]))
    valid = [b.bincode() for b in B.gen_config4(O.sign, rounds=5, n_auth=7, n_inc=5, n_vr=3)][-30:]
    out += [(name, b, valid[0][:64]) for name, b in count_attacks()]
    out += [(f"valid {i}", b, valid[(i + 1) % len(valid)][:64]) for i, b in enumerate(valid)]
    return out


def _oracle_form(st):
    """A statement of the test's reader in oracle/blocks.py's form."""
    ref = lambda r: B.BlockReference(*r)
    if st[0] == "share":
        return st
    if st[0] == "vote":
        return ("accept", B.Locator(ref(st[1]), st[2]))
    if st[0] == "reject":
        return ("reject", B.Locator(ref(st[1]), st[2]), None if st[3] is None else B.Locator(ref(st[3][0]), st[3][1]))
    return ("range", ref(st[1]), st[2], st[3])


class Packing:
    """The blocks in one buffer: block i starts at an offset congruent to i mod 8, its gap follows."""

    def __init__(self, all_cases, fill, copies=1):
        buf, offs, lens = bytearray(), [], []
        for _ in range(copies):
            for i, (_, b, cont) in enumerate(all_cases):
                pad = (i - len(buf)) % 8
                # (what aligns the next start belongs to the gap before it: the same fill)
                buf += self._fill(fill, pad, self._last_cont[GAP:] if offs else b"")
                offs.append(len(buf))
                lens.append(len(b))
                buf += b + self._fill(fill, GAP, cont)
                self._last_cont = cont
        self.buf = np.frombuffer(bytes(buf), dtype=np.uint8)
        self.offs, self.lens = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64)

    @staticmethod
    def _fill(fill, n, cont):
        return {"zeros": bytes(n), "ones": b"\xff" * n, "continuation": (cont + bytes(n))[:n]}[fill]


@pytest.fixture(scope="module")
def corpus():
    """The cases and the oracle's verdict on each one's own bytes, computed once."""
    cs = cases()
    assert 250 <= len(cs) <= 350
    pks, stakes, epoch = small_committee()
    bins = [b for _, b, _ in cs]
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(len(bins), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    st, md, bd = O.block_verify_batch(np.frombuffer(b"".join(bins) + b"\0", dtype=np.uint8), offs, lens, pks, stakes, epoch)
    st.flags.writeable = md.flags.writeable = bd.flags.writeable = False
    assert (st == O.BLOCK_OK).sum() >= 31 and (st == O.BLOCK_PARSE_ERROR).sum() >= 200
    return cs, (st, md, bd)


@pytest.fixture(scope="module")
def packings(corpus):
    return {fill: Packing(corpus[0], fill) for fill in FILLS}


@pytest.fixture(scope="module")
def own_engine():
    """An engine of the test's own for the calls that keep state (the index, the vote store)."""
    pks, stakes, epoch = small_committee()
    with M.Engine(devices=(0,)) as e:
        e.set_committee(pks, stakes, epoch)
        yield e


def same_as_oracle(got, want, names, what, copies=1):
    st, md, bd = (np.asarray(x) for x in got)
    ost, omd, obd = (np.concatenate([x] * copies) for x in want)
    bad = np.flatnonzero(st != ost)
    assert not len(bad), (what, names[bad[0] % len(names)], int(st[bad[0]]), int(ost[bad[0]]))
    ok = ost != O.BLOCK_PARSE_ERROR
    bad = np.flatnonzero(ok & ((md != omd).any(axis=1) | (bd != obd).any(axis=1)))
    assert not len(bad), (what, names[bad[0] % len(names)], "digests")


def to_device(p):
    import torch

    dev = torch.device("cuda", 0)
    i64 = lambda a: torch.from_numpy(a.view(np.int64).copy()).to(dev)
    return torch.from_numpy(p.buf.copy()).to(dev), i64(p.offs), i64(p.lens)


@pytest.mark.parametrize("fill", FILLS)
def test_host_buffer_verify(engine, corpus, packings, fill):
    cs, want = corpus
    pks, stakes, epoch = small_committee()
    engine.set_committee(pks, stakes, epoch)
    p = packings[fill]
    same_as_oracle(engine.verify_blocks_packed(p.buf, p.offs, p.lens), want, [c[0] for c in cs], fill)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("form", ["in_comb", "two_kernel", "separate_hash", "batch_walk", "batch_stage"])
def test_device_buffer_verify(engine, opts, corpus, packings, form, fill):
    """mv_dev_verify_blocks on the three small-call forms and, the packing repeated to MV_BATCH_MIN
    blocks, on both batch forms (the switches of tests/test_gpu_ingest.py)."""
    import torch

    cs, want = corpus
    opts("MV_HASH_IN_COMB", form != "separate_hash")
    opts("MV_INGEST_IN_COMB", form != "two_kernel")
    opts("MV_BLK_WALK", form != "batch_stage")
    pks, stakes, epoch = small_committee()
    engine.set_committee(pks, stakes, epoch)
    copies = -(-M.BATCH_MIN // len(cs)) if form.startswith("batch") else 1
    p = packings[fill] if copies == 1 else Packing(cs, fill, copies)
    d_buf, d_off, d_len = to_device(p)
    n = len(p.offs)
    dev = d_buf.device
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_md = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_bd = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # (the buffer's size includes the last gap, so every block has 16 readable bytes after it)
    engine.dev_verify_blocks(0, d_buf, int(p.offs[-1] + p.lens[-1]), d_off, d_len, d_st, d_md, d_bd)
    torch.cuda.synchronize()
    same_as_oracle((d_st.cpu().numpy(), d_md.cpu().numpy(), d_bd.cpu().numpy()), want, [c[0] for c in cs], (form, fill), copies)


@pytest.mark.parametrize("fill", FILLS)
def test_device_accept(own_engine, corpus, packings, fill):
    """mv_dev_accept_blocks over a cleared index: every block's status is the oracle's."""
    import torch

    cs, want = corpus
    e, p = own_engine, packings[fill]
    e.index_clear()
    e.index_reserve(4 * len(cs))
    d_buf, d_off, d_len = to_device(p)
    n = len(p.offs)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=d_buf.device)
    d_state = torch.full((n,), 255, dtype=torch.uint8, device=d_buf.device)
    torch.cuda.synchronize()
    e.dev_accept_blocks(0, d_buf, int(p.offs[-1] + p.lens[-1]), d_off, d_len, None, d_st, d_state, None)
    st = d_st.cpu().numpy()
    bad = np.flatnonzero(st != want[0])
    assert not len(bad), (fill, cs[bad[0]][0], int(st[bad[0]]), int(want[0][bad[0]]))


@pytest.mark.parametrize("fill", FILLS)
def test_device_votes(own_engine, corpus, packings, fill):
    """mv_dev_aggregate_votes, votes counted: statuses and counts are votes_model's over the
    statements of the blocks that parse."""
    import torch

    cs, want = corpus
    _, stakes, _ = small_committee()
    e, p = own_engine, packings[fill]
    e.votes_clear()
    e.votes_reserve(len(cs), 64 * len(cs))
    model = CellRule([int(s) for s in stakes])
    st_want, counts_want = [], []
    for (name, b, _), ost in zip(cs, want[0]):
        dec = decode_block(b)
        assert (dec is not None) == (ost != O.BLOCK_PARSE_ERROR), name
        if dec is None:
            st_want.append(M.VOTES_PARSE_ERROR)
            counts_want.append([0, 0, 0, 0])
            continue
        own, sts, _ = dec
        r = model.process_block((own[0], own, sts))
        st_want.append(M.VOTES_OK)
        counts_want.append([len(r.processed), r.unknown, r.duplicate, r.flags])
    d_buf, d_off, d_len = to_device(p)
    n = len(p.offs)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=d_buf.device)
    d_counts = torch.full((n, 4), -1, dtype=torch.int64, device=d_buf.device)
    d_cert = torch.zeros((256, 8), dtype=torch.int64, device=d_buf.device)
    torch.cuda.synchronize()
    total = e.dev_aggregate_votes(0, d_buf, int(p.offs[-1] + p.lens[-1]), d_off, d_len, d_st, d_counts, d_cert,
                                  register_only=False)
    assert d_st.cpu().numpy().tolist() == st_want, fill
    got = d_counts.cpu().numpy().tolist()
    bad = [i for i in range(n) if got[i] != counts_want[i]]
    assert not bad, (fill, cs[bad[0]][0], got[bad[0]], counts_want[bad[0]])
    assert total == sum(c[0] for c in counts_want)


@pytest.mark.parametrize("fill", FILLS)
def test_frames(engine, corpus, fill):
    """The same blocks as tag-1 frames, a stream each: behind the block's frame lies a second frame
    whose body begins with the gap's fill (for the continuation: with the bytes the block goes on
    with). Rows, block lists and block statuses are frames_model's, whose verdicts are the oracle's."""
    cs, _ = corpus
    com = small_committee()
    engine.set_committee(*com)
    buf, soff, slen = bytearray(), [], []
    for _, b, cont in cs:
        s = FM.frame(FM.blocks_msg(FM.TAG_BLOCKS, [b])) + FM.frame(Packing._fill(fill, 24, cont))
        soff.append(len(buf))
        slen.append(len(s))
        buf += s
    buf = np.frombuffer(bytes(buf) + bytes(GAP), dtype=np.uint8)
    got = engine.verify_frames_messages(buf, soff, slen)
    FM.assert_same(got, FM.model(buf, soff, slen, com), fill)
    assert len(got.blk_status) >= len(cs)
