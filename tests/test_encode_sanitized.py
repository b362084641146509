"""CPU: the rules of mv_encode_blocks under the host's AddressSanitizer and UBSan.

tools/encode_san.cpp includes the shipped encode_walk.h -- the payload check, the size pass, the
piece table -- and drives it word by word, the way k_en_write does. Every input array and the output
are heap allocations of exactly the size the contract grants, so a read or a write outside the
contract is a sanitizer report, which ends the run and fails the test. What it writes is compared
with tests/encode_model.py on the case lists of tests/encode_cases.py, the refused payloads included.

The harness is built with the host compiler and nothing is preloaded; if that compiler cannot link a
one-line sanitized program the test skips, every other build or run failure is a failure."""
import os
import shutil
import struct
import subprocess

import pytest

import encode_cases as C
import encode_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FLAGS = ["-std=c++17", "-O1", "-g"] + SAN
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("encode_san")
    if shutil.which(CXX) is None:
        pytest.skip(f"no host compiler {CXX}")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for link in (STATIC_RUNTIME, []):
        if subprocess.run([CXX] + SAN + link + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip(f"{CXX} cannot link a sanitized program")
    exe = d / "encode_san"
    r = subprocess.run([CXX] + FLAGS + link + [os.path.join(ROOT, "tools", "encode_san.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(call, cap):
        n, m, p = len(call.heads), len(call.includes), len(call.poff)
        src, dst = d / "in.bin", d / "out.bin"
        with open(src, "wb") as f:
            f.write(struct.pack("<5Q", n, m, p, len(call.pbuf), cap))
            f.write(struct.pack(f"<{10 * n}Q", *[w for h in call.heads for w in h]))
            f.write(struct.pack(f"<{6 * m}Q", *[w for row in call.includes for w in row]))
            f.write(struct.pack(f"<{p}Q", *call.poff) + struct.pack(f"<{p}Q", *call.plen))
            f.write(bytes(call.pbuf))
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, (call.name, r.returncode, r.stderr[-6000:])
        raw = open(dst, "rb").read()
        total, errors = struct.unpack_from("<2Q", raw)
        rows = struct.unpack_from(f"<{3 * n}Q", raw, 16)
        return total, errors, list(rows[0::3]), list(rows[1::3]), list(rows[2::3]), raw[16 + 24 * n:]

    return run


def check(harness, call):
    want = call.model()
    assert want.status == call.want
    total, errors, st, off, ln, out = harness(call, want.out_bytes)
    assert errors == 0 and total == want.out_bytes
    assert (st, off, ln) == (want.status, want.offs, want.lens)
    bad = [i for i, (o, l) in enumerate(zip(off, ln)) if out[o:o + l] != bytes(want.buf[o:o + l])]
    assert not bad, f"{call.name}: blocks differ from the model: {bad[:8]}"
    assert out == bytes(want.buf), "the padding"
    # a cap 8 bytes short: sizes and verdicts as before, no byte written
    if want.out_bytes >= 8:
        total, errors, st, off, ln, out = harness(call, want.out_bytes - 8)
        assert (total, errors, st, off, ln) == (want.out_bytes, 0, want.status, want.offs, want.lens)
        assert out == b"\xa5" * (want.out_bytes - 8)
    return want


def test_shapes(harness):
    want = check(harness, C.shapes())
    assert set(want.status) == {EM.OK}


def test_refusals(harness):
    c = C.refusals()
    want = check(harness, c)
    refused = {i for i, s in enumerate(want.status) if s != EM.OK}
    assert len(refused) >= 60 and all(want.lens[i] == 0 for i in refused)
    check(harness, c.without(refused))


def test_too_long(harness):
    want = check(harness, C.too_long())
    assert want.lens[0] == EM.MAX_LEN and want.status[1:4] == [EM.TOO_LONG, EM.TOO_LONG, EM.BAD_HEAD]
