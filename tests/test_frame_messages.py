"""CPU: mv_frame_messages, the host statement of the frame and message walk of mv_verify_frames
(handle_read_stream + the NetworkMessage decode, network.rs:400-457; RequestBlocks' limit,
net_sync.rs:282-285), against the pure-Python model of tests/frames_model.py: one row per message,
every block under its message, tags 0 / 2 / 4 bound-checked, and the walk stopped where the bytes
alone end the connection."""
import struct

import numpy as np
import pytest

import frames_model as FM
import mysticeti_amd as M
from frames_model import blocks_msg, frame, ping, ref, refs_msg, subscribe


def check(stream: bytes, what=""):
    got = M.frame_messages(stream)
    want = FM.model(stream, [0], [len(stream)])
    FM.assert_same(got, want, what)
    return got


def rand_blocks(rng, n):
    return [rng.integers(0, 256, size=int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for _ in range(n)]


def mixed_stream(rng):
    blks = rand_blocks(rng, 9)
    return (frame(subscribe()) + frame(blocks_msg(FM.TAG_BLOCKS, blks[:3])) + ping()
            + frame(refs_msg(FM.TAG_REQUEST, 2)) + frame(blocks_msg(FM.TAG_RESPONSE, blks[3:5])) + ping() + ping()
            + frame(blocks_msg(FM.TAG_BLOCKS, [])) + frame(refs_msg(FM.TAG_NOT_FOUND, 1))
            + frame(blocks_msg(FM.TAG_BLOCKS, blks[5:]) + b"trailing bytes are allowed")), blks


def test_constants_match_the_header():
    assert [M.MSG_OK, M.MSG_DECODE_ERROR, M.MSG_BLOCK_REJECTED, M.MSG_TOO_MANY_REQUESTED, M.MSG_NOT_REACHED,
            M.MSG_BAD_SIZE] == [FM.OK, FM.DECODE_ERROR, FM.BLOCK_REJECTED, FM.TOO_MANY_REQUESTED, FM.NOT_REACHED,
                                FM.BAD_SIZE]
    assert M.MSG_NONE == FM.NONE


def test_mixed_stream_of_all_tags_and_pings():
    stream, blks = mixed_stream(np.random.default_rng(3))
    got = check(stream)
    assert got.rows[:, 1].tolist() == [0, 1, 2, 3, 1, 4, 1] and (got.status == M.MSG_OK).all()
    assert got.rows[:, 5].tolist() == [0, 3, 0, 2, 0, 0, 4]
    assert int(got.consumed[0]) == len(stream) and got.drop_msg[0] == M.MSG_NONE
    assert [stream[int(o):int(o) + int(n)] for o, n in zip(got.blk_off, got.blk_len)] == blks
    # on a well-formed stream the block list is mv_frame_blocks's
    offs, lens, consumed = M.frame_blocks(stream)
    assert np.array_equal(offs, got.blk_off) and np.array_equal(lens, got.blk_len) and consumed == len(stream)


def test_every_truncation_of_a_two_frame_stream():
    rng = np.random.default_rng(4)
    a, b = rand_blocks(rng, 2), rand_blocks(rng, 3)
    whole = frame(blocks_msg(FM.TAG_BLOCKS, a)) + ping() + frame(blocks_msg(FM.TAG_RESPONSE, b))
    first = len(frame(blocks_msg(FM.TAG_BLOCKS, a)))
    for cut in range(len(whole) + 1):
        got = check(whole[:cut], cut)
        want_rows = 0 if cut < first else (1 if cut < len(whole) else 2)
        assert got.rows.shape[0] == want_rows, cut
        assert int(got.consumed[0]) == (0 if cut < first else first if cut < first + 12 else
                                        first + 12 if cut < len(whole) else len(whole)), cut


GOOD = frame(blocks_msg(FM.TAG_BLOCKS, [b"\x05" * 30, b"\x06" * 7]))
AFTER = frame(subscribe(3))  # never walked after a dropping frame

DROPS = {
    "size_above_16MiB": (struct.pack(">I", (16 << 20) + 1) + b"\0" * 8, FM.BAD_SIZE),
    "size_below_4": (frame(b"\x01\x00\x00"), FM.DECODE_ERROR),
    "tag_5": (frame(struct.pack("<IQ", 5, 0)), FM.DECODE_ERROR),
    **{f"tag_0_with_{n}_body_bytes": (frame(struct.pack("<I", 0) + b"\x07" * (n - 4)), FM.DECODE_ERROR)
       for n in range(4, 12)},
    "block_count_overrun": (frame(struct.pack("<IQ", 1, 2) + struct.pack("<Q", 4) + b"abcd"), FM.DECODE_ERROR),
    "block_length_overrun": (frame(struct.pack("<IQ", 3, 1) + struct.pack("<Q", 99) + b"short"), FM.DECODE_ERROR),
    "count_2_63": (frame(struct.pack("<IQ", 1, 1 << 63) + struct.pack("<Q", 4) + b"abcd"), FM.DECODE_ERROR),
    "count_2_63_refs": (frame(struct.pack("<IQ", 2, 1 << 63) + ref(1, 2)), FM.DECODE_ERROR),
    "reference_overrun_tag_2": (frame(refs_msg(2, 2, count=3)), FM.DECODE_ERROR),
    "reference_overrun_tag_4": (frame(refs_msg(4, 1)[:-1]), FM.DECODE_ERROR),
    "digest_length_31": (frame(struct.pack("<IQ", 2, 2) + ref(1, 2) + ref(2, 3, 31) + b"\0" * 40), FM.DECODE_ERROR),
    "digest_length_33": (frame(struct.pack("<IQ", 4, 1) + ref(1, 2, 33)), FM.DECODE_ERROR),
    "51_references_requested": (frame(refs_msg(2, 51)), FM.TOO_MANY_REQUESTED),
}


@pytest.mark.parametrize("case", sorted(DROPS))
def test_streams_the_reference_drops(case):
    bad, status = DROPS[case]
    stream = GOOD + ping() + bad + AFTER
    got = check(stream, case)
    assert got.status.tolist() == [FM.OK, status]
    assert got.drop_msg[0] == 1
    assert got.rows[1, 5] == 0 and got.rows[1, 7] == M.MSG_NONE  # lists no blocks, names none
    before = len(GOOD) + 12
    assert int(got.consumed[0]) == (before if status == FM.BAD_SIZE else before + len(bad))
    assert len(got.blk_off) == 2  # GOOD's two, nothing of the dropped frame
    # the same frames before the bad one are fine on their own
    assert (check(GOOD + ping()).status == FM.OK).all()


def test_request_of_50_is_served_and_51_is_not():
    ok = check(frame(refs_msg(2, 50)) + AFTER)
    assert ok.status.tolist() == [FM.OK, FM.OK]
    bad = check(frame(refs_msg(2, 51)) + AFTER)
    assert bad.status.tolist() == [FM.TOO_MANY_REQUESTED] and int(bad.consumed[0]) == len(frame(refs_msg(2, 51)))


def test_block_not_found_has_no_limit():
    got = check(frame(refs_msg(4, 51)) + AFTER)
    assert got.status.tolist() == [FM.OK, FM.OK]


def test_cap_smaller_than_the_counts_writes_the_first_and_counts_all():
    stream, blks = mixed_stream(np.random.default_rng(5))
    buf = np.frombuffer(stream, dtype=np.uint8)
    lib = M.load_library()
    import ctypes

    rows = np.zeros((2, 8), dtype=np.uint32)
    off = np.full(4, 77, dtype=np.uint64)
    ln = np.full(4, 77, dtype=np.uint64)
    nb, consumed = ctypes.c_uint64(0), ctypes.c_uint64(0)
    n = lib.mv_frame_messages(M._p(buf), buf.size, M._p(rows), 2, M._p(off), M._p(ln), 3, ctypes.byref(nb),
                              ctypes.byref(consumed))
    assert n == 7 and nb.value == 9 and consumed.value == len(stream)
    assert rows[:, 1].tolist() == [0, 1] and [int(x) for x in ln[:3]] == [len(b) for b in blks[:3]]
    assert int(off[3]) == 77 and int(ln[3]) == 77  # nothing past cap_blocks
    assert lib.mv_frame_messages(None, 5, None, 0, None, None, 0, None, None) == -1
    assert M.frame_messages(b"").rows.shape == (0, 8)


def test_random_bytes_agree_with_the_model():
    rng = np.random.default_rng(11)
    stream, _ = mixed_stream(rng)
    for k in range(300):
        if k % 2:
            b = rng.integers(0, 256, size=int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            if k % 4 == 1:  # a plausible size word in front
                b = struct.pack(">I", int(rng.integers(0, 64))) + b
        else:
            x = bytearray(stream)
            for _ in range(int(rng.integers(1, 4))):
                x[int(rng.integers(0, len(x)))] = int(rng.integers(0, 256))
            b = bytes(x)
        check(b, k)
