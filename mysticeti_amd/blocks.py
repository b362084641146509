"""Host-side StatementBlock builder for benchmark corpora (configs 1, 4 and 5).

Mirrors block creation in the reference, `StatementBlock::new_with_signer`
(mysticeti-core/src/types.rs:155-218): the signer signs BLAKE2b-256 of the digest
pre-image (`Signer::sign_block`, crypto.rs:199-223), and the block digest is
BLAKE2b-256(pre-image || signature) (`BlockDigest::new`, crypto.rs:38-61). The bytes
are the `Data<StatementBlock>` bincode encoding (types.rs:93-114, data.rs:43-52).

Signing goes through the engine's batched GPU signer (`Engine.ed25519_sign`, the f3 row
of SURVEY.md §8): every authority of a round is signed in one call. The pre-image and
bincode writers here are independent of oracle/ (the checker); tests compare the two.
"""
from __future__ import annotations

import hashlib
import struct
from typing import List, Sequence, Tuple

import numpy as np

# (authority, round, digest) -- BlockReference (types.rs:49-54)
Ref = Tuple[int, int, bytes]


def _ref_bin(r: Ref) -> bytes:
    return struct.pack("<QQQ", r[0], r[1], 32) + r[2]


def _ref_pre(r: Ref) -> bytes:  # CryptoHash of BlockReference: BE authority, BE round, digest
    return struct.pack(">QQ", r[0], r[1]) + r[2]


def encode(author: int, rnd: int, includes: Sequence[Ref], shares: Sequence[bytes],
           ranges: Sequence[Tuple[Ref, int, int]], time_ns: int, epoch: int, sig: bytes,
           digest: bytes) -> Tuple[bytes, bytes]:
    """(bincode, pre-image) of a block whose statements are the Shares, then the VoteRanges.

    Pre-image: crypto.rs:85-128 (Share = 0x00 || raw tx, types.rs:751-755; VoteRange =
    0x04 || block || BE start || BE end; u128 BE time; marker byte; BE epoch).
    """
    pre = [struct.pack(">QQ", author, rnd)]
    bn = [struct.pack("<QQQ", author, rnd, 32), digest, struct.pack("<Q", len(includes))]
    for r in includes:
        pre.append(_ref_pre(r))
        bn.append(_ref_bin(r))
    bn.append(struct.pack("<Q", len(shares) + len(ranges)))
    for tx in shares:
        pre.append(b"\x00" + tx)
        bn.append(struct.pack("<IQ", 0, len(tx)) + tx)
    for r, lo, hi in ranges:
        pre.append(b"\x04" + _ref_pre(r) + struct.pack(">QQ", lo, hi))
        bn.append(struct.pack("<I", 2) + _ref_bin(r) + struct.pack("<QQ", lo, hi))
    pre.append(struct.pack(">QQ", time_ns >> 64, time_ns & (2**64 - 1)) + b"\x00" + struct.pack(">Q", epoch))
    bn.append(struct.pack("<QQ", time_ns & (2**64 - 1), time_ns >> 64) + b"\x00" + struct.pack("<QQ", epoch, 64))
    bn.append(sig)
    return b"".join(bn), b"".join(pre)


def _b2(x: bytes) -> bytes:
    return hashlib.blake2b(x, digest_size=32).digest()


def genesis_refs(n_auth: int, epoch: int = 0) -> List[Ref]:
    """References of the genesis blocks (types.rs:141-150): round 0, no includes, zero signature."""
    out = []
    for a in range(n_auth):
        _, pre = encode(a, 0, [], [], [], 0, epoch, bytes(64), bytes(32))
        out.append((a, 0, _b2(pre + bytes(64))))
    return out


def authority_seed(a: int) -> bytes:
    return hashlib.sha512(b"mysti-auth" + struct.pack("<Q", a)).digest()[:32]


def config4_tx(r: int, a: int) -> bytes:
    """512-B Share tx (transactions_generator.rs:82-85): 8-B ts || 8-B rand || zeros."""
    return (1_700_000_000_000 + r).to_bytes(8, "little") + \
        ((r * 1_000_003 + a * 7919) & (2**64 - 1)).to_bytes(8, "little") + bytes(496)


def build_rounds(engine, rounds: int, n_auth: int, seeds: Sequence[bytes], n_inc: int, n_vr: int,
                 with_tx: bool, epoch: int = 0) -> List[bytes]:
    """Rounds 1..rounds of a DAG: each authority includes n_inc blocks of round r-1 (own
    first, core.rs:264-278), optionally one 512-B Share tx, and n_vr VoteRanges. One GPU
    signing call per round."""
    prev = genesis_refs(n_auth, epoch)
    seed_arr = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_auth, 32)
    out: List[bytes] = []
    for r in range(1, rounds + 1):
        specs, msgs = [], []
        for a in range(n_auth):
            others = [x for x in range(n_auth) if x != a]
            inc = [prev[a]] + [prev[x] for x in others[: n_inc - 1]]
            shares = [config4_tx(r, a)] if with_tx else []
            ranges = [(prev[(a + 1 + v) % n_auth], 0, 1 + (v % 7)) for v in range(n_vr)]
            t = r * 10**8 + a
            _, pre = encode(a, r, inc, shares, ranges, t, epoch, bytes(64), bytes(32))
            specs.append((a, inc, shares, ranges, t, pre))
            msgs.append(_b2(pre))
        _, sig = engine.ed25519_sign(seed_arr, np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(-1, 32))
        cur = []
        for (a, inc, shares, ranges, t, pre), s in zip(specs, sig):
            s = s.tobytes()
            d = _b2(pre + s)
            bn, _ = encode(a, r, inc, shares, ranges, t, epoch, s, d)
            out.append(bn)
            cur.append((a, r, d))
        prev = cur
    return out


def build_rounds_sealed(engine, rounds: int, n_auth: int, seeds: Sequence[bytes], n_inc: int, n_vr: int,
                        with_tx: bool, epoch: int = 0) -> List[bytes]:
    """build_rounds' DAG with the host out of the per-round loop: every round is encoded once with
    zero digests and signatures (the includes carry authority and round only), and one
    Engine.seal_blocks(link=True) call signs, digests and links all of them on the GPU
    (StatementBlock::new_with_signer, types.rs:155-218). Without VoteRanges (config 1) the result is
    build_rounds' byte for byte. The link rule covers includes, not the references inside
    statements, so the VoteRanges here name genesis blocks, whose digests are known up front, where
    build_rounds' name blocks of the round before: same sizes, same verdicts, other bytes."""
    gen = genesis_refs(n_auth, epoch)
    zero = bytes(32)
    out: List[bytes] = []
    for r in range(1, rounds + 1):
        prev = gen if r == 1 else [(a, r - 1, zero) for a in range(n_auth)]
        for a in range(n_auth):
            others = [x for x in range(n_auth) if x != a]
            inc = [prev[a]] + [prev[x] for x in others[: n_inc - 1]]
            shares = [config4_tx(r, a)] if with_tx else []
            ranges = [(gen[(a + 1 + v) % n_auth], 0, 1 + (v % 7)) for v in range(n_vr)]
            bn, _ = encode(a, r, inc, shares, ranges, r * 10**8 + a, epoch, bytes(64), zero)
            out.append(bn)
    lens = np.array([len(b) for b in out], dtype=np.uint64)
    offs = np.zeros(len(out), dtype=np.uint64)
    if len(out) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    buf = np.frombuffer(bytearray(b"".join(out)), dtype=np.uint8)
    st, _, _ = engine.seal_blocks(buf, offs, lens, np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_auth, 32),
                                  link=True)
    if st.any():
        raise RuntimeError(f"seal_blocks left {int(np.count_nonzero(st))} blocks unsealed")
    raw = buf.tobytes()
    return [raw[int(o): int(o) + int(l)] for o, l in zip(offs, lens)]


def _le_bytes(values, width: int) -> np.ndarray:
    """values (any integer array) as rows of `width` little-endian bytes."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    return v.view(np.uint8).reshape(v.shape + (8,))[..., :width]


def encoded_inputs(rounds: int, n_auth: int, n_inc: int, n_vr: int, with_tx: bool, epoch: int = 0):
    """The DAG of build_rounds_sealed as the inputs of Engine.encode_blocks, for all rounds at once and
    without a per-block loop: (heads [n, 10], includes [n k, 6], (payload bytes, offsets, lengths)).
    Block (r, a) is row (r - 1) n_auth + a; its includes are the own block of round r - 1 first, then
    the lowest other authorities (digest words: genesis' for round 1, zero above: the seal links them);
    its one payload is build_rounds_sealed's statements (none: no payload at all)."""
    n, k = rounds * n_auth, min(n_inc, n_auth)
    gen = genesis_refs(n_auth, epoch)
    gen_words = np.array([struct.unpack("<4Q", g[2]) for g in gen], dtype=np.uint64).reshape(n_auth, 4)
    a = np.tile(np.arange(n_auth, dtype=np.uint64), rounds)
    r = np.repeat(np.arange(1, rounds + 1, dtype=np.uint64), n_auth)
    n_st = (1 if with_tx else 0) + n_vr
    heads = np.zeros((n, 10), dtype=np.uint64)
    heads[:, 0], heads[:, 1], heads[:, 2], heads[:, 4] = a, r, r * np.uint64(10**8) + a, epoch
    heads[:, 6], heads[:, 7] = np.arange(n, dtype=np.uint64) * np.uint64(k), k
    if n_st:
        heads[:, 8], heads[:, 9] = np.arange(n, dtype=np.uint64), 1
    # include authorities of seat s: s, then the others in ascending order
    j = np.arange(1, k, dtype=np.int64)[None, :]
    seat = np.arange(n_auth, dtype=np.int64)[:, None]
    inc_auth = np.concatenate([seat, np.where(j - 1 < seat, j - 1, j)], axis=1)  # [n_auth, k]
    includes = np.zeros((rounds, n_auth, k, 6), dtype=np.uint64)
    includes[..., 0] = inc_auth[None]
    includes[..., 1] = np.arange(rounds, dtype=np.uint64)[:, None, None]
    if rounds:
        includes[0, :, :, 2:] = gen_words[inc_auth]
    includes = includes.reshape(n * k, 6)
    if not n_st:
        return heads, includes, (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    size = 8 + (524 if with_tx else 0) + 76 * n_vr
    pay = np.zeros((n, size), dtype=np.uint8)
    pay[:, 0:8] = _le_bytes(np.uint64(n_st), 8)
    at = 8
    if with_tx:  # Share(config4_tx(r, a)): tag 0, length 512, 8-B ts || 8-B rand || zeros
        pay[:, at + 4:at + 12] = _le_bytes(np.uint64(512), 8)
        pay[:, at + 12:at + 20] = _le_bytes(np.uint64(1_700_000_000_000) + r, 8)
        pay[:, at + 20:at + 28] = _le_bytes(r * np.uint64(1_000_003) + a * np.uint64(7919), 8)
        at += 524
    if n_vr:  # VoteRange(gen[(a + 1 + v) % n_auth], 0, 1 + v % 7): the same for every round
        v = np.arange(n_vr, dtype=np.int64)[None, :]
        target = (seat + 1 + v) % n_auth  # [n_auth, n_vr]
        vr = np.zeros((n_auth, n_vr, 76), dtype=np.uint8)
        vr[..., 0] = 2
        vr[..., 4:12] = _le_bytes(target, 8)
        vr[..., 20:28] = _le_bytes(np.uint64(32), 8)
        vr[..., 28:60] = gen_words[target].view(np.uint8).reshape(n_auth, n_vr, 32)
        vr[..., 68:76] = _le_bytes(1 + v % 7 + 0 * seat, 8)
        pay[:, at:] = np.tile(vr.reshape(n_auth, 76 * n_vr), (rounds, 1))
    offs = np.arange(n, dtype=np.uint64) * np.uint64(size)
    return heads, includes, (pay.reshape(-1), offs, np.full(n, size, dtype=np.uint64))


def build_rounds_encoded(engine, rounds: int, n_auth: int, seeds: Sequence[bytes], n_inc: int, n_vr: int,
                         with_tx: bool, epoch: int = 0) -> List[bytes]:
    """build_rounds_sealed's DAG, byte for byte, without the host encode: the heads, include rows and
    payloads of all rounds are numpy arrays (encoded_inputs), and one
    Engine.encode_blocks(seal=True, link=True) call writes the bincode, signs, digests and links it on
    the GPU (core.rs:264-291, types.rs:93-114, 155-218, data.rs:43-52)."""
    heads, includes, payloads = encoded_inputs(rounds, n_auth, n_inc, n_vr, with_tx, epoch)
    res = engine.encode_blocks(heads, includes, payloads, seal=True, link=True,
                               seeds=np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_auth, 32))
    if res.status.any() or res.seal_status.any():
        raise RuntimeError(f"encode_blocks left {int(np.count_nonzero(res.status | res.seal_status))} blocks unsealed")
    raw = res.buf.tobytes()
    return [raw[int(o): int(o) + int(l)] for o, l in zip(res.offs, res.lens)]


def config1(engine, rounds: int) -> List[bytes]:
    """Config 1: 4 authorities, all with the zero seed (dummy_signer, crypto.rs:355-357)."""
    return build_rounds(engine, rounds, 4, [bytes(32)] * 4, n_inc=4, n_vr=0, with_tx=False)


def config4(engine, rounds: int, n_auth: int = 100, n_inc: int = 67, n_vr: int = 66) -> List[bytes]:
    """Config-4 shape: 100 authorities with distinct seeds, 67 includes, one 512-B tx and 66
    VoteRanges (pre-image ~8,060 B, bincode ~9.5 KB)."""
    return build_rounds(engine, rounds, n_auth, [authority_seed(a) for a in range(n_auth)], n_inc, n_vr,
                        with_tx=True)


def committee(engine, n_auth: int, distinct: bool):
    """(pks[n][32], stakes) of a corpus committee, public keys derived on the GPU."""
    seeds = [authority_seed(a) if distinct else bytes(32) for a in range(n_auth)]
    pk, _ = engine.ed25519_sign(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(-1, 32),
                                np.zeros((n_auth, 32), dtype=np.uint8))
    return pk, np.ones(n_auth, dtype=np.uint64)


def pack(blocks: Sequence[bytes]):
    """(buf, off, len) arrays for Engine.verify_blocks_packed."""
    lens = np.array([len(b) for b in blocks], dtype=np.uint64)
    offs = np.zeros(len(blocks), dtype=np.uint64)
    if len(blocks) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    return np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8), offs, lens
