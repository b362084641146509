"""CPU: the case lists of the WAL write tests hit the edges they claim, and the layout rule that
mv_wal_layout and the kernels of mv_wal_write share (mysticeti_amd/csrc/wal_layout.h) agrees with the
oracle's writer on them.

The rule has two forms in that header: the entry-by-entry loop mv_wal_layout runs, and the prefix sum
with a step table that the kernels run. The second is driven here by tools/wal_write_san.cpp, built
with the host compiler (no sanitizer; test_wal_write_sanitized.py runs it under them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import wal as OW
import wal_write_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


def all_cases():
    cases = C.layout_edges() + C.own_alignment() + [C.append_case()]
    for s in range(8):
        cases += C.alignment(s)
    return cases


def gaps(case):
    """Per entry: the zero bytes the oracle put in front of it."""
    _, pos, _ = case.oracle()
    out, p = [], case.start
    for q, body in zip(pos, case.body_lens()):
        out.append(q - p)
        p = q + 16 + body
    return out, pos


def test_layout_edges_occur():
    by = {c.name: c for c in C.layout_edges()}
    m = 256
    g, pos = gaps(by["exact fill, the next entry on the boundary"])
    assert g == [0, 0, 0, 0] and pos[2] == m and (pos[1] + 16 + 124) == m
    g, pos = gaps(by["one byte longer: a gap"])
    assert g == [0, 140, 0, 0] and pos[1] == m
    g, pos = gaps(by["a whole map at a map start"])
    assert pos[0] == 0 and g[0] == 0 and pos[2] == 2 * m and g[2] == m - 21
    g, pos = gaps(by["a whole map from mid-map"])
    assert g == [0, m - 20, 0, 0] and pos[1:3] == [m, 2 * m]
    for name in ("every entry forces a gap", "gaps with own blocks"):
        g, pos = gaps(by[name])
        assert all(x > 0 for x in g[1:5 if "every" in name else 4]) and [p % m for p in pos[:4]] == [0] * 4
    g, pos = gaps(by["start mid-map"])
    assert pos[0] == 100 and sum(1 for x in g if x) == 2
    g, pos = gaps(by["start on a boundary"])
    assert pos[0] == 512 and g[0] == 0 and pos[1] == 768
    g, pos = gaps(by["start one byte before a boundary"])
    assert g[0] == 1 and pos[0] == 256
    g, pos = gaps(by["zero-length payloads"])
    assert not any(g) and pos[16] == m
    g, pos = gaps(by["a zero-length payload ends a map"])
    assert not any(g) and pos[1] == m
    g, pos = gaps(by["a zero-length payload straddles"])
    assert g == [15, 0, 0]
    assert by["n = 0"].oracle() == (b"", [], 77) and by["n = 1"].n == 1
    assert gaps(by["n = 1 with a gap"])[0] == [6]
    g, _ = gaps(by["the guessed window and the wide search"])
    assert by["the guessed window and the wide search"].n > 200 and sum(1 for x in g if x) > 5


def test_alignment_cases_cover_every_residue():
    seen = set()
    for s in range(8):
        for c in C.alignment(s):
            _, pos, _ = c.oracle()
            for (tag, off, ln, nxt), p in zip(c.rows, pos):
                assert off % 8 == s
                body_at = p + 16 + (8 if tag == C.OWN else 0)
                seen.add((ln, s, body_at % 8))
                seen.add(("kind", ln, (tag, nxt)))
    for ln in C.CRC_LENGTHS:
        assert all((ln, s, d) in seen for s in range(8) for d in range(8)), ln
        assert all(("kind", ln, k) in seen for k in C.KINDS), ln
    assert set(range(0, 21)) | set(range(251, 262)) | set(range(507, 518)) <= set(C.CRC_LENGTHS)
    assert sum(1 for x in C.CRC_LENGTHS if 1000 <= x <= 3100) >= 3
    own = set()
    for c in C.own_alignment():
        _, pos, _ = c.oracle()
        own |= {(nxt, off % 8, (p + 24) % 8) for (tag, off, ln, nxt), p in zip(c.rows, pos)}
    assert own == {(w, s, d) for w in C.NEXT_WORDS for s in range(8) for d in range(8)}


def test_refused_cases_are_what_they_say():
    for c in C.refused():
        bad = [i for i, ((tag, off, ln, _), body) in enumerate(zip(c.rows, c.body_lens()))
               if off + ln > len(c.buf) or body > (1 << c.map_bits) - 16]
        assert len(bad) == 1, c.name


def test_append_case_has_a_straddle_to_cut_at():
    c = C.append_case()
    g, _ = gaps(c)
    assert sum(1 for x in g if x) >= 3 and g[0] == 0


def test_wal_layout_equals_the_oracle():
    import mysticeti_amd as M

    for c in all_cases():
        _, pos, end = c.oracle()
        got, got_end = M.wal_layout(c.body_lens(), c.map_bits, c.start)
        assert got.tolist() == pos and got_end == end, c.name
    for bits, start, lens in C.random_lengths(11, 3000):
        w = OW.WalWriter(bits, bytes(start))
        pos = [w.write(1, bytes(n)) for n in lens]
        got, got_end = M.wal_layout(lens, bits, start)
        assert got.tolist() == pos and got_end == w.pos, (bits, start, lens)


@pytest.fixture(scope="module")
def plain_harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wal_write_plain")
    if shutil.which(CXX) is None:
        pytest.skip(f"no host compiler {CXX}")
    exe = d / "wal_write_plain"
    r = subprocess.run([CXX, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "wal_write_san.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return lambda calls: C.run_harness(exe, str(d), calls)


def test_the_step_table_form_equals_wal_layout(plain_harness):
    """The prefix sum with the crossing table, as the kernels run it, against mv_wal_layout: on the
    case lists and on a few thousand random length lists at map_bits 8-12 (cap 0: the layout alone)."""
    import mysticeti_amd as M

    calls = [(c, 0) for c in all_cases()]
    for k, (bits, start, lens) in enumerate(C.random_lengths(12, 3000)):
        calls.append((C.packed(f"random {k}", bits, start, lens, C.PLAIN, k % 8, seed=k), 0))
    res = plain_harness(calls)
    crossings = 0
    for (c, _), (refused, end, nc, pos, _) in zip(calls, res):
        want, want_end = M.wal_layout(c.body_lens(), c.map_bits, c.start)
        assert refused == 0 and pos == want.tolist() and end == want_end, c.name
        crossings += nc
    assert crossings > 3000
