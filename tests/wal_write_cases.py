"""The case lists of the WAL write tests (test_wal_write_cases.py, test_wal_write_sanitized.py,
test_gpu_wal_write.py). A Case is one mv_wal_write call: a payload buffer, n rows of tag | offset |
length | next_entry, the writer position and the map size. Its expected bytes come from
oracle/wal.py's WalWriter (zlib.crc32), written to a file of `start` zero bytes."""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

import numpy as np

import wal as OW

OWN = 3
NEXT_WORDS = (0, 1 << 63, 0x0807060504030201)
# what an entry is written as, in turn: the tags the reference knows but 3, an opaque one, and own
# blocks with the three next_entry words
KINDS = [(1, 0), (2, 0), (4, 0), (5, 0), (0xFFFFFFFF, 0)] + [(OWN, w) for w in NEXT_WORDS]
CRC_LENGTHS = list(range(0, 21)) + list(range(251, 262)) + list(range(507, 518)) + [1024, 2047, 3001]


class Case:
    def __init__(self, name: str, map_bits: int, start: int, buf: bytes, rows: Sequence[Tuple[int, int, int, int]]):
        self.name, self.map_bits, self.start, self.buf = name, map_bits, start, bytes(buf)
        self.rows = [tuple(int(x) for x in r) for r in rows]

    @property
    def n(self) -> int:
        return len(self.rows)

    def rows_array(self) -> np.ndarray:
        return np.array(self.rows, dtype=np.uint64).reshape(-1, 4)

    def body_lens(self) -> List[int]:
        return [ln + (8 if tag & 0xFFFFFFFF == OWN else 0) for tag, _, ln, _ in self.rows]

    def bodies(self) -> List[bytes]:
        return [(struct.pack("<Q", nxt) if tag & 0xFFFFFFFF == OWN else b"") + self.buf[off:off + ln]
                for tag, off, ln, nxt in self.rows]

    def oracle(self):
        """(the bytes appended behind `start`, positions, end_pos) from the oracle's writer."""
        w = OW.WalWriter(self.map_bits, bytes(self.start))
        pos = []
        for (tag, off, ln, nxt), body in zip(self.rows, self.bodies()):
            if tag & 0xFFFFFFFF == OWN:
                pos.append(w.writev(tag & 0xFFFFFFFF, [struct.pack("<Q", nxt), self.buf[off:off + ln]]))
            else:
                pos.append(w.write(tag & 0xFFFFFFFF, body))
        return w.image()[self.start:], pos, w.pos

    def slice(self, lo: int, hi: int, start: int) -> "Case":
        return Case(f"{self.name}[{lo}:{hi}]", self.map_bits, start, self.buf, self.rows[lo:hi])


def packed(name: str, map_bits: int, start: int, lens: Sequence[int], kinds=None, src_shift: int = 0, seed: int = 1,
           kind0: int = 0) -> Case:
    """Entries of these payload lengths, every payload at an offset = src_shift (mod 8) in a buffer
    of random bytes, the kinds taken in turn from `kinds` beginning with kind0."""
    kinds = KINDS if kinds is None else kinds
    rng = np.random.default_rng(seed)
    rows, off = [], src_shift
    for i, ln in enumerate(lens):
        tag, nxt = kinds[(kind0 + i) % len(kinds)]
        rows.append((tag, off, ln, nxt))
        off += ln
        off += (src_shift - off) % 8
    return Case(name, map_bits, start, rng.integers(0, 256, size=off + 3, dtype=np.uint8).tobytes(), rows)


PLAIN = [(1, 0)]


def layout_edges() -> List[Case]:
    """map_bits 8 (a map is 256 bytes): every edge of the position rule. Entry = payload + 16."""
    b = 8
    return [
        packed("exact fill, the next entry on the boundary", b, 0, [100, 124, 10, 7], PLAIN),  # 116 + 140 = 256
        packed("one byte longer: a gap", b, 0, [100, 125, 10, 7], PLAIN),
        packed("a whole map at a map start", b, 0, [240, 5, 240], PLAIN),
        packed("a whole map from mid-map", b, 0, [4, 240, 240, 3], PLAIN),
        packed("every entry forces a gap", b, 0, [150, 150, 150, 150, 150, 9], PLAIN),
        packed("gaps with own blocks", b, 0, [142, 142, 142, 142], [(OWN, 7)]),  # body 150
        packed("start mid-map", b, 100, [60, 60, 60, 60, 200, 1], PLAIN),
        packed("start on a boundary", b, 512, [240, 100, 124, 30], PLAIN),
        packed("start one byte before a boundary", b, 255, [0, 50, 174, 1], PLAIN),
        packed("zero-length payloads", b, 0, [0] * 20, PLAIN),  # sixteen fill a map exactly
        packed("a zero-length payload ends a map", b, 240, [0, 0, 3], PLAIN),
        packed("a zero-length payload straddles", b, 241, [0, 0, 3], PLAIN),
        packed("n = 0", b, 77, [], PLAIN),
        packed("n = 1", b, 0, [33], PLAIN),
        packed("n = 1 with a gap", b, 250, [33], PLAIN),
        packed("many small entries, mixed kinds", b, 3, [(7 * i) % 61 for i in range(150)], KINDS),
        packed("the guessed window and the wide search", b, 9, [1] * 90 + [200] * 8 + [0] * 120 + [111, 222] * 5, KINDS),
    ]


def alignment(src_shift: int) -> List[Case]:
    """map_bits 16 (no entry meets a boundary: a gap would fix its residue): the crc's row lengths and
    a few larger payloads, every payload at src_shift (mod 8) in the buffer; one case per writer
    position 0..7, so that over the eight cases every length is written at every destination
    residue; the kinds advance by one from case to case, so that every length also meets every kind
    over the eight source shifts."""
    return [packed(f"src {src_shift} dst {d}", 16, d, CRC_LENGTHS, KINDS, src_shift, seed=10 * src_shift + d,
                   kind0=src_shift + d) for d in range(8)]


def own_alignment() -> List[Case]:
    """Own blocks alone: every next_entry word at every source and destination residue (mod 8)."""
    out = []
    for s in range(8):
        for d in range(8):
            out.append(packed(f"own src {s} dst {d}", 9, d, [37, 0, 5, 260, 64, 3], [(OWN, w) for w in NEXT_WORDS], s,
                              seed=100 + 8 * s + d, kind0=s))
    return out


def refused() -> List[Case]:
    """Calls that mv_wal_write refuses with MV_E_INVALID_ARG: a body no map holds, a payload outside buf."""
    ok = [10, 20]
    big = packed("a body of 2^map_bits - 15", 8, 0, ok + [241], PLAIN)
    own = packed("an own block's body of 2^map_bits - 15", 8, 0, ok + [233], [(OWN, 1)])
    past = packed("a payload that ends past buf", 8, 0, ok + [30], PLAIN)
    past.rows[-1] = (1, len(past.buf) - 29, 30, 0)
    far = packed("a payload that starts past buf", 8, 0, ok + [0], PLAIN)
    far.rows[0] = (1, len(far.buf) + 1, 0, 0)
    wrap = packed("an offset that wraps", 8, 0, ok + [8], PLAIN)
    wrap.rows[1] = (1, (1 << 64) - 4, 8, 0)
    return [big, own, past, far, wrap]


def append_case() -> Case:
    return packed("append", 8, 40, [30, 90, 61, 0, 200, 17, 100, 100, 3, 230, 230, 12, 0, 55], KINDS, 3, seed=5)


def random_lengths(seed: int, count: int):
    """(map_bits, start, payload lengths) lists for the layout alone."""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        bits = int(rng.integers(8, 13))
        top = (1 << bits) - 16
        n = int(rng.integers(0, 60))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            lens = rng.integers(0, top + 1, size=n)
        elif kind == 1:
            lens = rng.integers(0, min(top, 64) + 1, size=n)
        else:
            lens = np.where(rng.integers(0, 4, size=n) == 0, top - rng.integers(0, 3, size=n), rng.integers(0, 40, size=n))
        yield bits, int(rng.integers(0, 4 << bits)), [int(x) for x in lens]


# ---- tools/wal_write_san.cpp: its input and output files
def harness_input(calls) -> bytes:
    """calls: (Case, cap) pairs."""
    parts = [struct.pack("<Q", len(calls))]
    for c, cap in calls:
        parts.append(struct.pack("<5Q", c.n, len(c.buf), c.start, c.map_bits, cap))
        parts.append(c.rows_array().tobytes())
        parts.append(c.buf)
    return b"".join(parts)


def harness_output(raw: bytes, calls):
    """Per call: (refused, end_pos, crossings, positions, the cap output bytes)."""
    out, at = [], 0
    for c, cap in calls:
        refused, end, nc = struct.unpack_from("<3Q", raw, at)
        pos = list(struct.unpack_from(f"<{c.n}Q", raw, at + 24))
        at += 24 + 8 * c.n
        out.append((refused, end, nc, pos, raw[at:at + cap]))
        at += cap
    assert at == len(raw)
    return out


def run_harness(exe, tmp_dir, calls):
    import os
    import subprocess

    src, dst = os.path.join(tmp_dir, "in.bin"), os.path.join(tmp_dir, "out.bin")
    with open(src, "wb") as f:
        f.write(harness_input(calls))
    r = subprocess.run([str(exe), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-6000:])
    with open(dst, "rb") as f:
        return harness_output(f.read(), calls)
