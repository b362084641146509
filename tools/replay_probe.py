"""What the device replay costs: mv_wal_replay against what a caller composes without it, on one image.

Input: N config-4-shape blocks (as bench_blocks.py builds them: 100 authorities, 67 includes, one
512-B Share, 66 VoteRanges) as WAL entries at 16-MiB maps (every 128th an own block, tag 3, the
rest tag 1) in one page-locked image (mv_host_alloc). Two paths over the same bytes, each warmed up
and then timed `--steps` times (the median is reported):

  new     mv_wal_replay: walk, crc, select, block verification, rows, cut and summary on the device
  parent  mv_wal_verify, a host pass (numpy) that lists the tag-1 / tag-3 payloads, mv_verify_blocks
          on them, and a host read (numpy gather) of the 56-byte references

Both are called through ctypes with preallocated outputs. Prints one JSON line.

    python tools/replay_probe.py [--blocks N] [--steps K] [--warmup W]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-bits", type=int, default=24)
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
    n_auth = 100
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)
    mark("corpus + committee")
    n, bits = a.blocks, a.map_bits
    own = lambda i: i % 128 == 5
    plen = np.array([len(base[i % len(base)]) + (8 if own(i) else 0) for i in range(n)], dtype=np.uint64)
    pos, end = M.wal_layout(plen, bits)
    image = eng.host_empty((end + 64,))
    image[:] = 0
    crcs = {}
    for i in range(n):
        b = base[i % len(base)]
        payload = (struct.pack("<Q", i) + b) if own(i) else b
        key = (i % len(base), own(i), i if own(i) else 0)
        if key not in crcs:
            crcs[key] = zlib.crc32(payload)
        p = int(pos[i])
        image[p:p + 16] = np.frombuffer(struct.pack("<QII", crcs[key], len(payload) + 16, 3 if own(i) else 1), dtype=np.uint8)
        image[p + 16:p + 16 + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    mark("image filled")
    lib, ctx, vp = eng.lib, eng.ctx, ctypes.c_void_p
    ptr = lambda x: vp(x.ctypes.data)
    cap = n + 8
    e_pos, e_tag = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    e_len, e_st = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
    rows, bst = np.zeros((cap, 10), dtype=np.uint64), np.zeros(cap, dtype=np.uint8)
    summary, seen = np.zeros(3, dtype=np.uint64), np.zeros(n_auth, dtype=np.uint64)
    cnt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def new():
        rc = lib.mv_wal_replay(ctx, ptr(image), end, end, bits, ptr(e_pos), ptr(e_tag), ptr(e_len), ptr(e_st), cap,
                               ctypes.byref(cnt), ptr(rows), ptr(bst), cap, ctypes.byref(nb), ptr(summary), ptr(seen))
        assert rc == 0 and cnt.value == n and nb.value == n, (rc, cnt.value, nb.value)

    p_pos, p_tag = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    p_len, p_st = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
    st2 = np.zeros(cap, dtype=np.uint8)
    c2 = ctypes.c_uint64(0)
    parent_out = {}

    def parent():
        rc = lib.mv_wal_verify(ctx, ptr(image), end, end, bits, ptr(p_pos), ptr(p_tag), ptr(p_len), ptr(p_st), cap,
                               ctypes.byref(c2))
        assert rc == 0 and c2.value == n, (rc, c2.value)
        k = c2.value
        is_own = p_tag[:k] == 3
        sel = np.flatnonzero(((p_tag[:k] == 1) | is_own) & (p_st[:k] == 0))
        skip = np.where(is_own[sel], 8, 0).astype(np.uint64)
        off = np.ascontiguousarray(p_pos[sel] + np.uint64(16) + skip)
        ln = np.ascontiguousarray(p_len[sel].astype(np.uint64) - skip)
        rc = lib.mv_verify_blocks(ctx, ptr(image), ptr(off), ptr(ln), len(sel), ptr(st2), None, None)
        assert rc == 0, rc
        refs = image[off[:, None].astype(np.int64) + np.arange(56)].view(np.uint64)  # authority, round, 32, digest
        parent_out.update(sel=sel, off=off, ln=ln, refs=refs)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    t_new, t_par = timed(new), timed(parent)
    mark("timed calls")
    # the checked calls: the two paths agree, and the new call's rows say what the image holds
    rows[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    bst[:] = 255
    new()
    parent()
    refs = parent_out["refs"]
    ok = bool(np.array_equal(e_pos[:n], p_pos[:n]) and np.array_equal(e_st[:n], p_st[:n]) and (e_st[:n] == 0).all()
              and np.array_equal(rows[:n, 0], parent_out["sel"].astype(np.uint64))
              and np.array_equal(rows[:n, 1], parent_out["off"]) and np.array_equal(rows[:n, 2], parent_out["ln"])
              and np.array_equal(rows[:n, 3:5], refs[:, 0:2]) and np.array_equal(rows[:n, 5:9], refs[:, 3:7])
              and np.array_equal(bst[:n], st2[:n]) and (bst[:n] == 0).all() and (bst[n:] == 255).all()
              and int(summary[0]) == int(refs[:, 1].max()) and int(summary[2]) == 0xFFFFFFFFFFFFFFFF
              and all(int(rows[i, 9]) == (i if own(i) else 0xFFFFFFFFFFFFFFFF) for i in range(0, n, 37)))
    # where the new call's time sits: the device stages (mv_stage_times) of one more call; the rest
    # is the image's copy, the replay kernels, the syncs and the copies back
    eng.set_stage_timing(True)
    eng.stage_times(reset=True)
    t0 = time.perf_counter()
    new()
    one_ms = (time.perf_counter() - t0) * 1e3
    stage_ms = {k: round(v, 3) for k, v in eng.stage_times(reset=True)[0].items() if v}
    eng.set_stage_timing(False)
    med = lambda v: round(float(np.median(v)), 3)
    print(json.dumps({"probe": "replay", "blocks": n, "map_bits": bits, "image_bytes": int(end),
                      "new_ms": {"median": med(t_new), "min": round(min(t_new), 3), "max": round(max(t_new), 3)},
                      "parent_ms": {"median": med(t_par), "min": round(min(t_par), 3), "max": round(max(t_par), 3)},
                      "new_blocks_per_s": round(n / med(t_new) * 1e3), "parent_blocks_per_s": round(n / med(t_par) * 1e3),
                      "new_image_GB_per_s": round(end / med(t_new) / 1e6, 2),
                      "parent_image_GB_per_s": round(end / med(t_par) / 1e6, 2),
                      "staged_call_ms": round(one_ms, 3), "staged_call_stages_ms": stage_ms,
                      "phase_s": {b[0]: round(b[1] - a_[1], 3) for a_, b in zip(stamps, stamps[1:])},
                      "results_equal_and_ok": ok, "steps": a.steps, "warmup": a.warmup}))
    eng.host_free(image)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
