"""CPU: the layout rules of mv_wal_write under the host's AddressSanitizer and UBSan.

tools/wal_write_san.cpp includes the shipped wal_layout.h -- the checks, the crossing steps, the step
table, the spans and the header words -- and drives it in the order the kernels do. Rows, payload
bytes, positions and the output are heap allocations of exactly the size the contract grants, so a
read or a write outside the contract is a sanitizer report, which ends the run and fails the test.
What it writes is compared byte for byte with the oracle's writer (oracle/wal.py, zlib.crc32) on the
case lists of tests/wal_write_cases.py, the refused calls included.

The harness is built with the host compiler and nothing is preloaded; if that compiler cannot link a
one-line sanitized program the test skips, every other build or run failure is a failure."""
import os
import shutil
import subprocess

import pytest

import wal_write_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FLAGS = ["-std=c++17", "-O1", "-g"] + SAN
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]
CANARY = 64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("wal_write_san")
    if shutil.which(CXX) is None:
        pytest.skip(f"no host compiler {CXX}")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for link in (STATIC_RUNTIME, []):
        if subprocess.run([CXX] + SAN + link + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip(f"{CXX} cannot link a sanitized program")
    exe = d / "wal_write_san"
    r = subprocess.run([CXX] + FLAGS + link + [os.path.join(ROOT, "tools", "wal_write_san.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return lambda calls: C.run_harness(exe, str(d), calls)


def check(harness, cases):
    want = [c.oracle() for c in cases]
    exact = harness([(c, len(w[0])) for c, w in zip(cases, want)])
    roomy = harness([(c, len(w[0]) + CANARY) for c, w in zip(cases, want)])
    short = harness([(c, len(w[0]) - 1) for c, w in zip(cases, want) if w[0]])
    for c, (img, pos, end), e, r in zip(cases, want, exact, roomy):
        assert e[:2] == (0, end) and e[3] == pos and e[4] == img, c.name
        assert r[3] == pos and r[4] == img + b"\xa5" * CANARY, c.name
    for (c, (img, pos, end)), s in zip([(c, w) for c, w in zip(cases, want) if w[0]], short):
        assert s[:2] == (0, end) and s[3] == pos and s[4] == b"\xa5" * (len(img) - 1), c.name


def test_layout_edges(harness):
    check(harness, C.layout_edges() + [C.append_case()])


def test_alignment(harness):
    check(harness, [c for s in range(8) for c in C.alignment(s)] + C.own_alignment())


def test_refused(harness):
    cases = C.refused()
    for c, (refused, end, _, _, out) in zip(cases, harness([(c, 512) for c in cases])):
        assert refused == 1 and end == c.start and out == b"\xa5" * 512, c.name
