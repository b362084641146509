"""What the device frame walk costs: mv_verify_frames against the path it replaces, on one arena.

Input: N config-4-shape blocks (as bench_blocks.py builds them: 100 authorities, 67 includes, one
512-B Share, 66 VoteRanges) in Blocks frames of 100 blocks, spread over 99 streams (n - 1 peers of
a 100-node committee) in one page-locked arena (mv_host_alloc). Two paths over the same bytes,
each warmed up and then timed `--steps` times (the median is reported):

  new     mv_verify_frames: frame walk, message walk, block verification, verdicts on the device
  parent  mv_frame_blocks per stream on the host, then one mv_verify_blocks on the listed blocks

Both are called through ctypes with preallocated outputs. Prints one JSON line.

    python tools/frames_probe.py [--blocks N] [--steps K] [--warmup W]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=99)
    ap.add_argument("--frame-blocks", type=int, default=100)
    a = ap.parse_args()
    stamps = [("start", time.perf_counter())]
    mark = lambda what: stamps.append((what, time.perf_counter()))
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    mark("imports")
    eng = M.Engine(devices=(0,))
    mark("mv_create")
    base = MB.config4(eng, rounds=41)  # 4,100 distinct blocks
    pks, stakes = MB.committee(eng, 100, distinct=True)
    eng.set_committee(pks, stakes, 0)
    mark("corpus + committee")
    n, ns, fb = a.blocks, a.streams, a.frame_blocks
    # stream s holds blocks [cut[s], cut[s + 1]) in frames of fb
    cut = [n * s // ns for s in range(ns + 1)]
    frames = []  # (stream, first block, count)
    for s in range(ns):
        for i in range(cut[s], cut[s + 1], fb):
            frames.append((s, i, min(fb, cut[s + 1] - i)))
    lens = np.array([len(base[i % len(base)]) for i in range(n)], dtype=np.int64)
    pre = np.concatenate([[0], np.cumsum(lens + 8)])
    total = int(pre[-1]) + 16 * len(frames)
    arena = eng.host_empty((total + 64,))
    soff, slen = np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint64)
    p, cur = 0, -1
    for s, i, k in frames:
        if s != cur:
            if cur >= 0:
                slen[cur] = p - int(soff[cur])
            soff[s], cur = p, s
        body = 12 + int(pre[i + k] - pre[i])
        hdr = struct.pack(">I", body) + struct.pack("<IQ", 1, k)
        arena[p:p + 16] = np.frombuffer(hdr, dtype=np.uint8)
        p += 16
        for j in range(i, i + k):
            b = base[j % len(base)]
            arena[p:p + 8] = np.frombuffer(struct.pack("<Q", len(b)), dtype=np.uint8)
            arena[p + 8:p + 8 + len(b)] = np.frombuffer(b, dtype=np.uint8)
            p += 8 + len(b)
    slen[cur] = p - int(soff[cur])
    assert p == total
    mark("arena filled")
    lib, ctx, vp = eng.lib, eng.ctx, ctypes.c_void_p
    ptr = lambda x: vp(x.ctypes.data)
    consumed, drop = np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint32)
    rows = np.zeros((len(frames), 8), dtype=np.uint32)
    off, ln, st = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    nm, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def new():
        rc = lib.mv_verify_frames(ctx, ptr(arena), ptr(soff), ptr(slen), ns, ptr(consumed), ptr(drop), ptr(rows),
                                  len(frames), ctypes.byref(nm), ptr(off), ptr(ln), ptr(st), n, ctypes.byref(nb))
        assert rc == 0 and nm.value == len(frames) and nb.value == n, (rc, nm.value, nb.value)

    off2, ln2, st2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    c2 = ctypes.c_uint64(0)

    def parent():
        k = 0
        for s in range(ns):
            o = int(soff[s])
            got = lib.mv_frame_blocks(vp(arena.ctypes.data + o), int(slen[s]), vp(off2.ctypes.data + 8 * k),
                                      vp(ln2.ctypes.data + 8 * k), n - k, ctypes.byref(c2))
            assert got >= 0
            off2[k:k + got] += np.uint64(o)
            k += got
        assert k == n
        rc = lib.mv_verify_blocks(ctx, ptr(arena), ptr(off2), ptr(ln2), n, ptr(st2), None, None)
        assert rc == 0, rc

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    # interleaved rounds would hide nothing here: both paths are synchronous host calls
    t_new, t_par = timed(new), timed(parent)
    mark("timed calls")
    # the checked calls: every output starts from a sentinel, so an entry left unwritten shows
    for x in (st, st2):
        x[:] = 255
    for x in (off, ln, off2, ln2, consumed):
        x[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    rows[:] = 0xFFFFFFFF
    drop[:] = 7
    new()
    parent()
    unset = np.uint64(0xFFFFFFFFFFFFFFFF)
    untouched = int((st == 255).sum() + (st2 == 255).sum() + (off == unset).sum() + (off2 == unset).sum()
                    + (rows[:, 0] == 0xFFFFFFFF).sum())
    ok = bool(untouched == 0 and (st == 0).all() and (st2 == 0).all() and np.array_equal(off, off2)
              and np.array_equal(ln, ln2) and (rows[:, 6] == 0).all() and np.array_equal(consumed, slen)
              and (drop == 0xFFFFFFFF).all() and int(ln.sum()) == int(lens.sum()))
    # where the new call's time sits: the block pipeline's device stages (mv_stage_times) of one
    # more call; the rest is the arena's copy, the walk kernels, their two syncs and the copies back
    eng.set_stage_timing(True)
    eng.stage_times(reset=True)
    t0 = time.perf_counter()
    new()
    one_ms = (time.perf_counter() - t0) * 1e3
    stage_ms = {k: round(v, 3) for k, v in eng.stage_times(reset=True)[0].items() if v}
    eng.set_stage_timing(False)
    med = lambda v: round(float(np.median(v)), 3)
    print(json.dumps({"probe": "frames", "blocks": n, "streams": ns, "frames": len(frames), "arena_bytes": total,
                      "new_ms": {"median": med(t_new), "min": round(min(t_new), 3), "max": round(max(t_new), 3)},
                      "parent_ms": {"median": med(t_par), "min": round(min(t_par), 3), "max": round(max(t_par), 3)},
                      "new_blocks_per_s": round(n / med(t_new) * 1e3), "parent_blocks_per_s": round(n / med(t_par) * 1e3),
                      "staged_call_ms": round(one_ms, 3), "staged_call_block_stages_ms": stage_ms,
                      "new_arena_GB_per_s": round(total / med(t_new) / 1e6, 2),
                      "parent_arena_GB_per_s": round(total / med(t_par) / 1e6, 2),
                      "outputs_left_at_sentinel": untouched,
                      "phase_s": {b[0]: round(b[1] - a_[1], 3) for a_, b in zip(stamps, stamps[1:])},
                      "results_equal_and_ok": ok, "steps": a.steps, "warmup": a.warmup}))
    eng.host_free(arena)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
