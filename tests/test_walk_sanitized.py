"""CPU: the byte walkers of the library under the host's AddressSanitizer and UBSan.

tools/walk_san.cpp includes the shipped walker code -- bincode_walk.h (block_walk), ingest_lane.h
(ingest_lane), votes_walk.h (the votes statement walk), frame_walk.h, wal_entry.h, block_ref.h -- and
links block_codec.cpp. It gives every walker its input in a heap allocation of exactly the size
the walker's contract grants, so a read or a write outside the contract is a sanitizer report, which
ends the run and fails the test. What the walkers print is compared with the C oracle
(StatementBlock::verify), hashlib's BLAKE2b, frames_model and, where no buffer is involved,
big-integer restatements of the headers' rules.

votes_model takes statements, not bytes: the statements the votes walker is compared with come from
a strict bincode reader written here (a reader that fails when a read runs past the block, as
frames_model's does), in votes_cases' form; it is itself held to the oracle's parse verdict.

The harness is built with the host compiler and nothing is preloaded; if that compiler cannot link a
one-line sanitized program the test skips, every other build or run failure is a failure."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import blocks as B
import frames_model as FM
import lane_kinds as K
import mysticeti_amd as M
import oracle as O
import preimage_edges as E
from walk_cases import U64, count_attacks, decode_block, every_kind_block, small_committee

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the build line of the harness
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", "-O1", "-g"] + SAN
# the sanitizer runtimes inside the program where the compiler can (gcc links them as shared libraries
# by default, which have to come first among a process's libraries): the program then runs the same
# whatever else its environment loads
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]
SOURCES = [os.path.join(ROOT, "tools", "walk_san.cpp"), os.path.join(ROOT, "mysticeti_amd", "csrc", "block_codec.cpp")]

# facts word (block_verdict.h)
BF_PARSED, BF_EPOCH_OK, BF_AUTHOR_OK, BF_GENESIS, BF_QUORUM, BF_INC_SHIFT, BF_VR_SHIFT = 1, 2, 4, 8, 32, 8, 16
VR_STATUS = {0: 0, 1: O.BLOCK_VOTE_RANGE, 2: O.BLOCK_VOTE_RANGE_TOO_LONG, 3: O.BLOCK_VOTE_RANGE_END_TOO_LARGE}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_san")
    if shutil.which(CXX) is None:
        pytest.skip(f"no host compiler {CXX}")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for link in (STATIC_RUNTIME, []):
        if subprocess.run([CXX] + SAN + link + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip(f"{CXX} cannot link a sanitized program")
    exe = d / "walk_san"
    r = subprocess.run([CXX] + FLAGS + link + SOURCES + ["-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (args[0], r.returncode, r.stderr[-6000:])
        return r.stdout.splitlines()

    run.dir = d
    return run


def write_corpus(path, records):
    with open(path, "wb") as f:
        for b in records:
            f.write(struct.pack("<I", len(b)) + b)


def write_committee(path, stakes, epoch):
    stakes = [int(s) for s in stakes]
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQ", len(stakes), epoch, 2 * sum(stakes) // 3) + struct.pack(f"<{len(stakes)}Q", *stakes))


def _key(ref):
    return f"{ref[0]},{ref[1]}," + "".join(f"{w:016x}" for w in struct.unpack("<4Q", ref[2]))


def votes_line(decoded):
    """What the harness prints for the votes walker of a block that decodes."""
    own, sts, _ = decoded
    out = [f"votes=1 n_st={len(sts)} own={_key(own)}"]
    for k, st in enumerate(sts):
        if st[0] == "share":
            out.append(f"s{k}")
        elif st[0] == "vote":
            out.append(f"v{k}:{_key(st[1])}:{st[2]}")
        elif st[0] == "reject":
            out.append(f"j{k}")
        else:
            out.append(f"r{k}:{_key(st[1])}:{st[2]}:{st[3]}")
    return " ".join(out)


# ---------------------------------------------------------------- the block groups
def verdict(epoch_ok, author_ok, genesis, inc, vr, quorum):
    """StatementBlock::verify after the digest (types.rs:333-374), the signature taken as valid."""
    if not epoch_ok:
        return O.BLOCK_EPOCH_MISMATCH
    if not author_ok:
        return O.BLOCK_UNKNOWN_AUTHOR
    if genesis:
        return O.BLOCK_GENESIS
    return inc or vr or (O.BLOCK_OK if quorum else O.BLOCK_THRESHOLD_CLOCK)


def fields(line):
    """A harness line as {section: {key: value}}; sections: walk, lane, votes (its text), codec, P."""
    assert line.startswith("B "), line[:80]
    idx, d, rest = line[2:].split(" ", 2)
    body, _, p = rest.rpartition(" P=")
    out = {"idx": int(idx), "d": d, "P": bytes.fromhex(p)}
    head, _, codec = body.partition(" codec=")
    head, _, votes = head.partition(" votes=")
    walk, _, lane = head.partition(" lane ")
    out["votes"] = "votes=" + votes
    for name, text in (("walk", walk), ("lane", lane), ("codec", "codec=" + codec)):
        out[name] = dict(t.split("=", 1) for t in text.split(" ") if "=" in t)
        out[name + "_flags"] = [t for t in text.split(" ") if t and "=" not in t]
    return out


def check_blocks(lines, bins, committee, what):
    """Every line of one harness run against the oracle's StatementBlock::verify of the same bytes."""
    pks, stakes, epoch = committee
    n_auth = len(stakes)
    assert len(lines) == len(bins), (what, len(lines), len(bins))
    for i, (line, b, (ost, omd, obd)) in enumerate(zip(lines, bins, oracle_of(bins, committee))):
        f = fields(line)
        at = (what, i, len(b))
        assert f["idx"] == i and f["d"] == "d=*", (at, "the alignments disagree", line[:300])
        assert not f["walk_flags"] and not f["lane_flags"] and not f["codec_flags"], (at, line[:300])
        parsed = ost != O.BLOCK_PARSE_ERROR
        decoded = decode_block(b)
        assert (decoded is not None) == parsed, (at, "the test's own reader against the oracle")
        want = "1" if parsed else "0"
        assert f["walk"]["walk"] == want and f["walk"]["gather"] == want and f["codec"]["codec"] == want, at
        if not parsed:
            assert f["lane"]["pre_len"] == "0" and f["lane"]["facts"] == "0" and f["P"] == b"", at
            assert f["votes"] == "votes=0", at
            continue
        P = f["P"]
        assert hashlib.blake2b(P, digest_size=32).digest() == omd, (at, "B2(P)")
        assert int(f["walk"]["plen"]) == len(P) and int(f["walk"]["sig_pos"]) == decoded[2] - 64, at
        # the one-lane ingest: P || sig || 8 zero bytes inside the block's own span, the facts word
        lane = f["lane"]
        sig = bytes.fromhex(lane["sig"])
        assert lane["P"] == "gather" and int(lane["pre_len"]) == len(P) and lane["pre_off"] == "0" and lane["zero"] == "00" * 8, at
        assert hashlib.blake2b(P + sig, digest_size=32).digest() == obd, (at, "B2(P || sig)")
        assert bytes.fromhex(lane["claimed"]) == b[24:56], at
        fw = int(lane["facts"])
        assert fw & BF_PARSED, at
        inc, vr = (fw >> BF_INC_SHIFT) & 0xFF, VR_STATUS[(fw >> BF_VR_SHIFT) & 3]
        sig_reached = bool(fw & BF_EPOCH_OK) and bool(fw & BF_AUTHOR_OK) and not fw & BF_GENESIS
        assert bytes.fromhex(lane["sig_out"]) == (sig if sig_reached else sig[:32] + b"\xff" * 32), at
        assert int(lane["key"]) == (struct.unpack_from("<Q", b)[0] if fw & BF_AUTHOR_OK else 0), at
        got = verdict(fw & BF_EPOCH_OK, fw & BF_AUTHOR_OK, fw & BF_GENESIS, inc, vr, fw & BF_QUORUM)
        # the host codec: the same pre-image, signature and facts
        c = f["codec"]
        assert c["P"] == "gather" and int(c["plen"]) == len(P) and bytes.fromhex(c["sig"]) == sig, at
        assert bytes.fromhex(c["claimed"]) == b[24:56], at
        got_c = verdict(int(c["epoch"]) == epoch, int(c["author"]) < n_auth, int(c["round"]) == 0, int(c["inc"]), int(c["vr"]),
                        c["quorum"] == "1")
        for name, g, reached in (("lane", got, sig_reached), ("codec", got_c, got_c not in (O.BLOCK_EPOCH_MISMATCH,
                                                                                             O.BLOCK_UNKNOWN_AUTHOR,
                                                                                             O.BLOCK_GENESIS))):
            if ost == O.BLOCK_DIGEST_MISMATCH:  # decided ahead of every fact
                continue
            if ost == O.BLOCK_SIG_INVALID:  # decided after epoch, author and genesis, ahead of the rest
                assert reached, (at, name, g)
            else:
                assert g == ost, (at, name, g, ost)
        assert f["votes"] == votes_line(decoded), (at, f["votes"][:200], votes_line(decoded)[:200])
    return len(lines)


def oracle_of(bins, committee):
    pks, stakes, epoch = committee
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(len(bins), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    st, md, bd = O.block_verify_batch(np.frombuffer(b"".join(bins) + b"\0", dtype=np.uint8), offs, lens, pks, stakes, epoch)
    return [(int(st[i]), md[i].tobytes(), bd[i].tobytes()) for i in range(len(bins))]


def flips_and_garbage():
    """The byte-flip and garbage lists of test_gpu_ingest.py, by the same seed."""
    base = [b.bincode() for b in B.gen_config4(O.sign, rounds=2, n_auth=7, n_inc=5, n_vr=3)]
    rng = np.random.default_rng(21)
    out = []
    for _ in range(1500):
        b = bytearray(base[int(rng.integers(0, len(base)))])
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    for _ in range(300):
        out.append(rng.integers(0, 256, size=int(rng.integers(0, 700)), dtype=np.uint8).tobytes())
    return out + base


def test_blocks_at_every_alignment(harness):
    """block_walk (parse only and gathering P), ingest_lane, the votes walker and parse_block over the
    pre-image edge corpus, the one-lane kinds, the flip and garbage lists and the count attacks, each
    block at d = 0..7 (a corpus block's stated alignment is one of them)."""
    d = harness.dir
    n = {}
    cases = E.corpus()
    write_corpus(d / "edges.bin", [c.bincode for c in cases])
    com = E.committee()
    write_committee(d / "edges.com", com[1], com[2])
    n["preimage_edges"] = check_blocks(harness("blocks", d / "edges.bin", d / "edges.com"), [c.bincode for c in cases], com,
                                       "preimage_edges")
    assert n["preimage_edges"] == 1549

    small = small_committee()
    write_committee(d / "small.com", small[1], small[2])
    groups = {"lane_kinds": list(K.corpus()[0]), "flips_and_garbage": flips_and_garbage(),
              "count_attacks": [b for _, b in count_attacks()]}
    assert K.committee()[1].tolist() == small[1].tolist()
    for name, bins in groups.items():
        write_corpus(d / f"{name}.bin", bins)
        n[name] = check_blocks(harness("blocks", d / f"{name}.bin", d / "small.com"), bins, small, name)
    # the attacks do what they are named after: all but the valid block and the counts that fit fail
    st = [o[0] for o in oracle_of(groups["count_attacks"], small)]
    assert st[0] == O.BLOCK_OK and sum(s == O.BLOCK_PARSE_ERROR for s in st) >= len(st) - 4
    print("blocks per group:", n)


def test_every_prefix(harness):
    """Every prefix of the block of every statement kind and of a block with a 9-KB Share, at
    d = 0..7: none but the whole block parses, and none is read or written outside its span."""
    d = harness.dir
    small = small_committee()
    write_committee(d / "small.com", small[1], small[2])
    whole = [every_kind_block()[0], every_kind_block(9000)[0]]
    write_corpus(d / "whole.bin", whole)
    bins = [b[:k] for b in whole for k in range(len(b) + 1)]
    lines = harness("prefixes", d / "whole.bin", d / "small.com")
    assert check_blocks(lines, bins, small, "prefixes") == sum(len(b) + 1 for b in whole)
    parsed = [i for i, l in enumerate(lines) if " walk=1" in l]
    assert parsed == [len(whole[0]), len(bins) - 1]
    print("prefixes:", len(lines))


# ---------------------------------------------------------------- frames
def frame_streams():
    rng = np.random.default_rng(9)
    blks = [rng.integers(0, 256, size=int(rng.integers(0, 120)), dtype=np.uint8).tobytes() for _ in range(7)]
    fr, body16 = FM.frame, bytes(range(16))
    out = {"mixed": (fr(FM.subscribe()) + fr(FM.blocks_msg(FM.TAG_BLOCKS, blks[:3])) + FM.ping()
                     + fr(FM.refs_msg(FM.TAG_REQUEST, 2)) + fr(FM.blocks_msg(FM.TAG_RESPONSE, blks[3:5])) + FM.ping()
                     + fr(FM.blocks_msg(FM.TAG_BLOCKS, [])) + fr(FM.refs_msg(FM.TAG_NOT_FOUND, 1))
                     + fr(FM.blocks_msg(FM.TAG_BLOCKS, blks[5:]) + b"trailing bytes are allowed"))}
    for size in (0, 1, 3, 4, FM.MAX_SIZE, FM.MAX_SIZE + 1):
        out[f"size word {size}"] = struct.pack(">I", size) + body16 + fr(FM.subscribe())
    rem = 200
    for tag, unit in ((FM.TAG_BLOCKS, 8), (FM.TAG_RESPONSE, 8), (FM.TAG_REQUEST, 56), (FM.TAG_NOT_FOUND, 56)):
        for count in (rem // unit + 1, rem // unit, U64, 1 << 63):
            out[f"tag {tag} count {count}"] = fr(struct.pack("<IQ", tag, count) + bytes(rem)) + fr(FM.subscribe())
    out["block length to the frame's end"] = fr(struct.pack("<IQQ", 1, 1, 30) + bytes(30))
    out["block length one past the frame's end"] = fr(struct.pack("<IQQ", 1, 1, 31) + bytes(30)) + fr(FM.subscribe())
    out["block length 2^64 - 1"] = fr(struct.pack("<IQQ", 3, 1, U64) + bytes(30))
    for n in (50, 51):
        out[f"request of {n}"] = fr(FM.refs_msg(FM.TAG_REQUEST, n)) + fr(FM.subscribe())
        out[f"not found of {n}"] = fr(FM.refs_msg(FM.TAG_NOT_FOUND, n))
    for tag in (FM.TAG_REQUEST, FM.TAG_NOT_FOUND):  # the stream ends with the reference's 56 bytes
        bad = struct.pack("<QQQ", 1, 2, 31) + bytes(32)
        out[f"tag {tag}: a last reference of digest length 31"] = fr(struct.pack("<IQ", tag, 2) + FM.ref(3, 4) + bad)
        assert out[f"tag {tag}: a last reference of digest length 31"][-56:] == bad
    return out


def test_frames_every_prefix(harness):
    """frame_at and classify stepped over every prefix of each stream, the allocation exactly the
    prefix: rows, block lists and consumed bytes are frames_model's."""
    d = harness.dir
    streams = frame_streams()
    write_corpus(d / "frames.bin", list(streams.values()))
    lines = harness("frame-prefixes", d / "frames.bin")
    cases = [(name, s[:k]) for name, s in streams.items() for k in range(len(s) + 1)]
    assert len(lines) == len(cases)
    seen = set()
    for i, (line, (name, s)) in enumerate(zip(lines, cases)):
        at = (name, len(s))
        head, *rows = line.split(" | ")
        assert head.split(" ")[:2] == ["F", str(i)], at
        want_rows, want_consumed = FM.walk_stream(s)
        assert int(head.split("consumed=")[1]) == want_consumed, (at, head)
        # the device walk lists the frames after the one that ends the connection too; k_stream_cut drops them
        assert len(rows) >= len(want_rows), (at, line[:300])
        for text, want in zip(rows, want_rows):
            t = text.split(" ")
            kv = dict(x.split("=") for x in t[:5])
            blocks = [tuple(int(v) for v in x.split(":")) for x in t[5:]]
            assert int(kv["off"]) == want["off"] and int(kv["tag"]) == want["tag"] and int(kv["status"]) == want["status"], \
                (at, text[:200], want)
            seen.add(want["status"])
            end = want["off"] + 4 + int(kv["size"])
            if want["status"] == FM.OK:
                assert int(kv["nblk"]) == len(want["blocks"]), (at, text[:200])
                assert blocks == [(k, o, n) for k, (o, n) in enumerate(want["blocks"])], (at, text[:200])
            else:
                assert int(kv["nblk"]) == 0, (at, text[:200])
            if want["status"] != FM.BAD_SIZE:  # what the sink saw lies inside the frame, decoded or not
                assert all(o <= end and n <= end - o for _, o, n in blocks) and end <= len(s), (at, text[:200])
    assert seen == {FM.OK, FM.DECODE_ERROR, FM.TOO_MANY_REQUESTED, FM.BAD_SIZE}
    print("frame streams:", len(streams), "prefixes:", len(cases))


# ---------------------------------------------------------------- wal_entry.h and block_ref.h: values only
def edge_values(size):
    vals = {0, 1, 15, 16, 17, (1 << 32) - 1, (1 << 32) + 1, (1 << 64) - 17, U64}
    return sorted(vals | {v for v in (size - 16, size - 15) if v >= 0})


def wal_rule(tag, pos, plen, size):
    """wal_entry.h's comment in unbounded integers: (status, block, off, len)."""
    if not 1 <= tag <= 5:
        return M.WAL_UNKNOWN_TAG, 0, 0, 0
    if tag not in (1, 3):
        return M.WAL_OK, 0, 0, 0
    skip = 8 if tag == 3 else 0  # OwnBlockData's next_entry
    if plen < skip or pos + 16 + plen > size:  # the header and the payload lie inside the image
        return M.WAL_BLOCK_DECODE, 0, 0, 0
    return M.WAL_OK, 1, pos + 16 + skip, plen - skip


def test_wal_and_reference_rules_do_not_wrap(harness):
    d = harness.dir
    sizes = sorted({0, 1, 15, 16, 17, 4096, (1 << 32) - 1, (1 << 32) + 1, (1 << 64) - 17, U64})
    wal = [(tag, pos, plen, size) for size in sizes for pos in edge_values(size) for plen in edge_values(size)
           for tag in range(7)]
    lens = sorted(set(edge_values(4096)) | {55, 56, 57, 63, 64, 65, 64 + 55, 64 + 56, 64 + 57})
    refs = [(ln, k) for ln in lens for k in lens]
    with open(d / "sweep.txt", "w") as f:
        f.writelines(f"w {t} {p} {l} {s}\n" for t, p, l, s in wal)
        f.writelines(f"r {ln} {k}\n" for ln, k in refs)
    lines = harness("sweep", d / "sweep.txt")
    assert len(lines) == len(wal) + len(refs) + 1
    for line, (tag, pos, plen, size) in zip(lines, wal):
        want = wal_rule(tag, pos, plen, size)
        assert line == f"w {tag} {pos} {plen} {size} -> " + " ".join(str(v) for v in want), (line, want)
        assert want[2] + want[3] <= size  # (the rule itself: a block it admits lies inside the image)
    for line, (ln, k) in zip(lines[len(wal):], refs):
        # block_ref.h: the own reference is bytes 0..56, the count at 56..64, include j at 64 + 56 j
        inside = int(64 + 56 * k <= ln) if ln >= 64 else -1
        want = f"r {ln} {k} -> {int(ln >= 56)} {int(ln >= 64)} {inside} {(64 + 56 * k) & U64}"
        assert line == want, (line, want)
    assert lines[-1] == "k 0 8 24 32 40 48"  # a key: the reference without its length word
    print("wal entries:", len(wal), "reference cases:", len(refs))
