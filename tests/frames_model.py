"""Helper (not a test): what the reference does with one connection's received bytes, message by
message, restated in plain Python for the tests of mv_frame_messages / mv_verify_frames.

  handle_read_stream   network.rs:400-447: a u32 big-endian size, 0 = a ping with 8 more bytes,
                       above MAX_SIZE = 16 MiB the connection is dropped; then
                       bincode::deserialize::<NetworkMessage> (network.rs:36-46, 454-457), which
                       decodes every inner Data<StatementBlock> (data.rs:83-96) and ends the
                       connection on any error
  connection_task      net_sync.rs:272-312: RequestBlocks above MAXIMUM_BLOCK_REQUEST = 50 ends it
  process_blocks       net_sync.rs:314-383: Err at the first rejected block, before add_blocks

The decoder below reads as bincode does (a reader that fails when a read runs past the frame); it
shares nothing with the library's walk. Block verdicts come from the CPU oracle
(oracle.block_verify_batch). The stream builders the tests use live here too."""
import struct

import numpy as np

import oracle as O

MAX_SIZE = 16 << 20
MAX_REQUEST = 50
OK, DECODE_ERROR, BLOCK_REJECTED, TOO_MANY_REQUESTED, NOT_REACHED, BAD_SIZE = range(6)
NONE = 0xFFFFFFFF
TAG_SUBSCRIBE, TAG_BLOCKS, TAG_REQUEST, TAG_RESPONSE, TAG_NOT_FOUND = range(5)


# ---- builders -------------------------------------------------------------------------------
def frame(body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + body


def ping() -> bytes:
    return struct.pack(">I", 0) + struct.pack("<q", 12345)


def blocks_msg(tag: int, blocks) -> bytes:
    out = struct.pack("<IQ", tag, len(blocks))
    for b in blocks:
        out += struct.pack("<Q", len(b)) + b
    return out


def ref(a: int, r: int, dlen: int = 32) -> bytes:  # BlockReference: authority, round, digest
    return struct.pack("<QQQ", a, r, dlen) + bytes([a & 0xFF]) * dlen


def refs_msg(tag: int, n: int, count=None) -> bytes:
    return struct.pack("<IQ", tag, n if count is None else count) + b"".join(ref(k, k + 1) for k in range(n))


def subscribe(rnd: int = 17) -> bytes:
    return struct.pack("<IQ", TAG_SUBSCRIBE, rnd)


# ---- the model -------------------------------------------------------------------------------
class _DecodeError(Exception):
    pass


class _Reader:
    def __init__(self, b: bytes):
        self.b, self.p = b, 0

    def take(self, n: int) -> int:
        if n > len(self.b) - self.p:
            raise _DecodeError()
        at = self.p
        self.p += n
        return at

    def u32(self) -> int:
        return struct.unpack_from("<I", self.b, self.take(4))[0]

    def u64(self) -> int:
        return struct.unpack_from("<Q", self.b, self.take(8))[0]


def decode_message(body: bytes):
    """bincode::deserialize::<NetworkMessage> as far as the frame decides it: (tag, [(offset in
    body, length) of each Data<StatementBlock>], number of BlockReferences). Raises _DecodeError."""
    r = _Reader(body)
    tag = r.u32()
    blocks, nrefs = [], 0
    if tag == TAG_SUBSCRIBE:
        r.u64()
    elif tag in (TAG_BLOCKS, TAG_RESPONSE):
        for _ in range(r.u64()):  # bincode reads element after element until one does not fit
            ln = r.u64()
            blocks.append((r.take(ln), ln))
    elif tag in (TAG_REQUEST, TAG_NOT_FOUND):
        nrefs = r.u64()
        for _ in range(nrefs):
            r.u64()
            r.u64()
            dl = r.u64()
            r.take(dl)
            if dl != 32:  # "Invalid block digest length" (crypto.rs:322-334)
                raise _DecodeError()
    else:
        raise _DecodeError()
    return tag, blocks, nrefs


def walk_stream(b: bytes):
    """One connection: ([row dicts: tag, off, status, blocks [(off, len)]], consumed). Stops where the
    bytes alone end the connection."""
    rows, p, consumed = [], 0, 0
    while len(b) - p >= 4:
        size = struct.unpack_from(">I", b, p)[0]
        if size > MAX_SIZE:
            rows.append(dict(tag=NONE, off=p, status=BAD_SIZE, blocks=[]))
            break
        need = size if size else 8
        if len(b) - p - 4 < need:
            break
        if size == 0:
            p += 12
            consumed = p
            continue
        body = b[p + 4:p + 4 + size]
        row = dict(tag=struct.unpack_from("<I", body)[0] if size >= 4 else NONE, off=p, status=OK, blocks=[])
        try:
            tag, blocks, nrefs = decode_message(body)
            row["blocks"] = [(p + 4 + o, ln) for o, ln in blocks]
            if tag == TAG_REQUEST and nrefs > MAX_REQUEST:
                row["status"] = TOO_MANY_REQUESTED
        except _DecodeError:
            row["status"] = DECODE_ERROR
        rows.append(row)
        p += 4 + size
        consumed = p
        if row["status"] != OK:
            break
    return rows, consumed


class Result:
    def __init__(self, rows, consumed, drop_msg, blk_off, blk_len, blk_status):
        self.rows, self.consumed, self.drop_msg = rows, consumed, drop_msg
        self.blk_off, self.blk_len, self.blk_status = blk_off, blk_len, blk_status

    @property
    def status(self):
        return self.rows[:, 6] & 0xFF


def model(buf, soff, slen, committee=None) -> Result:
    """The expected result of mv_verify_frames(buf, soff, slen); committee = (pks, stakes, epoch).
    committee None: the host-only walk (mv_frame_messages): no block verdicts."""
    raw = bytes(buf)
    rows, consumed, blk_off, blk_len, owner = [], [], [], [], []
    for s, (o, n) in enumerate(zip(soff, slen)):
        o, n = int(o), int(n)
        srows, c = walk_stream(raw[o:o + n])
        consumed.append(c)
        for r in srows:
            rows.append([s, r["tag"], (o + r["off"]) & 0xFFFFFFFF, (o + r["off"]) >> 32, len(blk_off), len(r["blocks"]),
                         r["status"], NONE])
            for bo, bl in r["blocks"]:
                blk_off.append(o + bo)
                blk_len.append(bl)
    rows = np.array(rows, dtype=np.uint32).reshape(-1, 8)
    blk_off = np.array(blk_off, dtype=np.uint64)
    blk_len = np.array(blk_len, dtype=np.uint64)
    blk_status = None
    if committee is not None:
        pks, stakes, epoch = committee
        blk_status = np.zeros(0, dtype=np.uint8)
        if len(blk_off):
            blk_status = O.block_verify_batch(np.frombuffer(raw + b"\0", dtype=np.uint8), blk_off, blk_len, pks, stakes,
                                              epoch)[0]
        for r in rows:
            if r[6] != OK:
                continue
            st = blk_status[int(r[4]):int(r[4]) + int(r[5])]
            unparsable = np.flatnonzero(st == O.BLOCK_PARSE_ERROR)
            rejected = np.flatnonzero(st != O.BLOCK_OK)
            if len(unparsable):  # the message does not deserialize: before any block is verified
                r[6], r[7] = DECODE_ERROR | (O.BLOCK_PARSE_ERROR << 8), unparsable[0]
            elif len(rejected):
                r[6], r[7] = BLOCK_REJECTED | (int(st[rejected[0]]) << 8), rejected[0]
    drop = np.full(len(soff), NONE, dtype=np.uint32)
    for i, r in enumerate(rows):
        s = int(r[0])
        if drop[s] != NONE:
            r[6], r[7] = NOT_REACHED, NONE
        elif r[6] & 0xFF:
            drop[s] = i
    return Result(rows, np.array(consumed, dtype=np.uint64), drop, blk_off, blk_len, blk_status)


def assert_same(got, want, what=""):
    """got (mysticeti_amd.FrameVerdicts) equals the model's Result, field by field."""
    assert got.rows.shape == want.rows.shape, (what, got.rows.shape, want.rows.shape)
    bad = np.flatnonzero((got.rows != want.rows).any(axis=1))
    assert not len(bad), (what, int(bad[0]), got.rows[bad[0]].tolist(), want.rows[bad[0]].tolist())
    assert np.array_equal(got.consumed, want.consumed), (what, "consumed")
    assert np.array_equal(got.drop_msg, want.drop_msg), (what, "drop_msg")
    assert np.array_equal(got.blk_off, want.blk_off), (what, "blk_off")
    assert np.array_equal(got.blk_len, want.blk_len), (what, "blk_len")
    if want.blk_status is not None:
        assert np.array_equal(got.blk_status, want.blk_status), (what, "blk_status")
