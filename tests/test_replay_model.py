"""CPU: the model the GPU tests of mv_wal_replay compare against (tests/replay_model.py, the replay
loop of BlockStore::open, block_store.rs:50-116) on hand-written images with expected values written
out here. The images come from oracle/wal.py's WalWriter over fixed bytes; the blocks are stand-ins
(a 56-byte reference and a tail), and so are their verdicts: the byte after the reference is the
MV_BLOCK_* the stand-in reports, and anything too short for a reference does not parse."""
import struct

import numpy as np

import oracle as O
import replay_model as RM
import wal as W

N_AUTH = 4
NONE = RM.NONE


def fake(authority, rnd, fill, status=0, dlen=32):
    return struct.pack("<QQQ", authority, rnd, dlen) + bytes([fill]) * 32 + bytes([status]) + b"tail"


def stand_in(img, offs, lens):
    out = []
    for o, l in zip(offs.tolist(), lens.tolist()):
        if l < 57 or struct.unpack_from("<Q", img, o + 16)[0] != 32:
            out.append(O.BLOCK_PARSE_ERROR)
        else:
            out.append(int(img[o + 56]))
    return np.array(out, dtype=np.uint8)


def run(w, end=None):
    return RM.model(w.image(), w.pos if end is None else end, w.map_bits, N_AUTH, stand_in)


def base_writer():
    w = W.WalWriter(16)
    w.write(1, fake(1, 5, 0x11))
    w.write(2, b"payload!")
    w.write(1, fake(2, 9, 0x22, status=O.BLOCK_SIG_INVALID))
    w.write(3, struct.pack("<Q", 0x0102030405060708) + fake(1, 7, 0x33))
    w.write(4, b"state")
    return w


def test_hand_written_image():
    r = run(base_writer())
    assert r.pos.tolist() == [0, 77, 101, 178, 263]
    assert r.tag.tolist() == [1, 2, 1, 3, 4]
    assert r.len.tolist() == [61, 8, 61, 69, 5]
    assert r.status.tolist() == [0, 0, 0, 0, 0] and (r.count, r.n_blocks) == (5, 3)
    assert r.rows.tolist() == [
        [0, 16, 61, 1, 5] + [0x1111111111111111] * 4 + [NONE],
        [2, 117, 61, 2, 9] + [0x2222222222222222] * 4 + [NONE],
        [3, 202, 61, 1, 7] + [0x3333333333333333] * 4 + [0x0102030405060708],
    ]
    # a rejected block is a row like any other: the reference's replay does not verify
    assert r.blk_status.tolist() == [O.BLOCK_OK, O.BLOCK_SIG_INVALID, O.BLOCK_OK]
    assert r.summary.tolist() == [9, 2, 4]
    assert r.last_seen.tolist() == [0, 7, 9, 0]


def test_empty_and_no_blocks():
    r = run(W.WalWriter(16))
    assert (r.count, r.n_blocks) == (0, 0) and r.summary.tolist() == [0, NONE, NONE] and r.last_seen.tolist() == [0] * 4
    w = W.WalWriter(16)
    w.write(5, b"commit")
    w.write(4, b"")
    w.write(2, b"x")
    r = run(w)
    assert (r.count, r.n_blocks) == (3, 0) and r.summary.tolist() == [0, NONE, 1]


def test_unknown_tags_stop_the_replay():
    for t in (0, 6):
        w = base_writer()
        w.write(t, b"what")
        w.write(1, fake(3, 50, 0x44))
        r = run(w)
        assert r.count == 6 and r.status.tolist() == [0] * 5 + [RM.UNKNOWN_TAG] and r.tag[5] == t
        assert r.n_blocks == 3 and r.summary.tolist() == [9, 2, 4] and r.last_seen.tolist() == [0, 7, 9, 0]


def test_own_block_payload_of_0_to_8_bytes():
    """Under 8 bytes the OwnBlockData header does not read; at 8 it reads and an empty block
    follows, which does not decode either (block_store.rs:531, 534)."""
    for n in range(9):
        w = W.WalWriter(16)
        w.write(1, fake(0, 3, 0x55))
        w.write(3, bytes(range(1, n + 1)))
        w.write(4, b"late state")
        r = run(w)
        assert r.status.tolist() == [0, RM.BLOCK_DECODE], n
        assert (r.count, r.n_blocks) == (2, 1) and r.summary.tolist() == [3, NONE, NONE] and r.last_seen.tolist() == [3, 0, 0, 0]


def test_decode_comes_before_the_authority_check():
    w = W.WalWriter(16)
    w.write(1, fake(N_AUTH, 8, 0x66))  # decodes, authority = committee size
    r = run(w)
    assert r.status.tolist() == [RM.UNKNOWN_AUTHORITY] and r.n_blocks == 0 and r.last_seen.tolist() == [0] * 4
    w = W.WalWriter(16)
    w.write(1, fake(N_AUTH + 9, 8, 0x66, dlen=31))  # does not decode, and its authority is outside too
    r = run(w)
    assert r.status.tolist() == [RM.BLOCK_DECODE] and r.n_blocks == 0
    w = W.WalWriter(16)
    w.write(3, struct.pack("<Q", 77) + fake(N_AUTH - 1, 8, 0x66))  # the largest authority inside
    r = run(w)
    assert r.status.tolist() == [0] and r.rows[0, 3] == 3 and r.rows[0, 9] == 77 and r.summary.tolist() == [8, 0, NONE]


def test_the_earliest_failing_entry_wins():
    def image(bad_crc_at):
        w = W.WalWriter(16)
        pos = [w.write(1, fake(k % 4, k + 1, k)) for k in range(5)]
        pos.append(w.write(1, fake(1, 99, 0x77, dlen=5)))  # entry 5 does not decode
        pos += [w.write(2, b"p" * 9), w.write(1, fake(2, 100, 0x78))]
        img = bytearray(w.image())
        img[pos[bad_crc_at] + 16 + 60] ^= 1  # the payload's last byte: parses as before, crc differs
        return RM.model(bytes(img), w.pos, 16, N_AUTH, stand_in)

    r = image(7)  # a crc failure after the decode failure: the list ends at 5
    assert r.count == 6 and r.status.tolist() == [0] * 5 + [RM.BLOCK_DECODE] and r.n_blocks == 5
    assert r.summary.tolist() == [5, NONE, NONE] and r.last_seen.tolist() == [5, 2, 3, 4]
    r = image(3)  # ... and one before it: the list ends at 3, with the crc status
    assert r.count == 4 and r.status.tolist() == [0] * 3 + [RM.CRC_MISMATCH] and r.n_blocks == 3
    assert r.rows[:, 0].tolist() == [0, 1, 2] and r.summary.tolist() == [3, NONE, NONE] and r.last_seen.tolist() == [1, 2, 3, 0]


def test_a_block_past_the_end_of_the_file_is_a_decode_failure():
    """A file cut inside a block whose missing tail is zeros keeps its crc (the mapping reads zeros
    there, wal.rs:226-261) but the library reads no block past the image."""
    w = W.WalWriter(16)
    w.write(2, b"before")
    w.write(1, fake(1, 5, 0x11) + bytes(20))
    img = w.image()[:-7]
    r = RM.model(img, w.pos, 16, N_AUTH, stand_in)
    assert r.status.tolist() == [0, RM.BLOCK_DECODE] and r.n_blocks == 0
