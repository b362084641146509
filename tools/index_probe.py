"""What the index costs: mv_accept_blocks against the parent's mv_verify_blocks on one arena.

Input: N config-4-shape blocks (100 authorities, 67 includes, one 512-B Share, 66 VoteRanges), all
distinct -- N / 100 rounds of one DAG in delivery order, in 100-block groups (one round, one
message) -- in one page-locked arena (mv_host_alloc). That is a catching-up node's traffic: every
block is new and every include (67 N lookups of a 48-byte key) is a block of the same call or of
the genesis round. Four legs over the same bytes, each warmed up and then timed `--steps` times
(the median is reported), the whole measurement `--runs` times:

  parent      mv_verify_blocks (what a caller of the parent commit runs before its own hash maps)
  accept      mv_accept_blocks on an index that holds the genesis references only
  half_known  mv_accept_blocks with every second block's reference seeded as HAVE: those blocks are
              skipped ahead of verify

  device      the same two calls on the arena's copy in HBM (mv_dev_verify_blocks + a stream
              synchronise against mv_dev_accept_blocks): no copy of the bytes in either, so the
              difference is the index work with its kernels, scans and host round trips

Between accept calls the index is cleared and seeded again (not timed), so each call does the same
work. One more call of each leg runs under mv_set_stage_timing: the device time of the block
pipeline's stages for these blocks (the device leg's, one pass), against which the index work
(device accept - device verify) is held. Prints one JSON line.

    python tools/index_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    stamps = [("start", time.perf_counter())]
    mark = lambda what: stamps.append((what, time.perf_counter()))
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    mark("imports")
    eng = M.Engine(devices=(0,))
    n_auth, n = 100, a.blocks
    bins = MB.config4(eng, rounds=(n + n_auth - 1) // n_auth)[:n]
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)
    mark("corpus + committee")
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum((lens + np.uint64(7)) & ~np.uint64(7))[:-1]
    total = int(offs[-1] + lens[-1])
    arena = eng.host_empty((total + 64,))
    arena[:] = 0
    for o, b in zip(offs.tolist(), bins):
        arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    grp = (np.arange(n, dtype=np.uint64) // np.uint64(100)).astype(np.uint64)
    own = np.ascontiguousarray(arena[offs[:, None].astype(np.int64) + np.arange(56)].view(np.uint64)[:, [0, 1, 3, 4, 5, 6]])
    includes = int(sum(int.from_bytes(b[56:64], "little") for b in bins))
    genesis = M.ref_words(MB.genesis_refs(n_auth))
    mark("arena filled")
    lib, ctx, vp = eng.lib, eng.ctx, ctypes.c_void_p
    ptr = lambda x: vp(x.ctypes.data)
    st, state, st_p = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    cap = 1024
    miss = np.zeros((cap, 6), dtype=np.uint64)
    nm = ctypes.c_uint64(0)
    eng.index_reserve(2 * n + n_auth)

    def seed(half):
        eng.index_clear()
        eng.index_insert(genesis, M.REF_HAVE)
        if half:
            eng.index_insert(own[1::2], M.REF_HAVE)

    def parent():
        rc = lib.mv_verify_blocks(ctx, ptr(arena), ptr(offs), ptr(lens), n, ptr(st_p), None, None)
        assert rc == 0 and not st_p.any(), rc

    def accept():
        rc = lib.mv_accept_blocks(ctx, ptr(arena), ptr(offs), ptr(lens), ptr(grp), n, ptr(st), ptr(state), ptr(miss), cap,
                                  ctypes.byref(nm))
        assert rc == 0, (rc, lib.mv_last_error(ctx))

    def timed(fn, before=None):
        ms = []
        for k in range(a.warmup + a.steps):
            if before:
                before()
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def staged(fn, before=None):
        if before:
            before()
        eng.set_stage_timing(True)
        eng.stage_times(reset=True)
        fn()
        out = {k: round(v, 3) for k, v in eng.stage_times(reset=True)[0].items() if v}
        eng.set_stage_timing(False)
        return out

    # the arena in HBM: the block path and the accept call without the copy of the bytes
    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(np.asarray(arena)).to(dev)
    t64 = lambda x: torch.from_numpy(x.view(np.int64).copy()).to(dev)
    d_off, d_len, d_grp = t64(offs), t64(lens), t64(grp)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_miss = torch.zeros((cap, 6), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    dev_nm = [0]

    def dev_parent():
        eng.dev_verify_blocks(0, d_arena, total, d_off, d_len, d_st)
        torch.cuda.synchronize(dev)

    def dev_accept():
        dev_nm[0] = eng.dev_accept_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss)

    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    runs, ok = [], True
    for _ in range(a.runs):
        t_par = timed(parent)
        t_acc = timed(accept, lambda: seed(False))
        ok &= bool((state == M.ACC_NEW).all() and not st.any() and nm.value == 0)
        s_acc = eng.index_stats()
        t_half = timed(accept, lambda: seed(True))
        ok &= bool((state[1::2] == M.ACC_KNOWN).all() and (state[0::2] == M.ACC_NEW).all() and not st.any())
        # an even block's includes of odd blocks are HAVE; those of even blocks arrive in the same call
        ok &= nm.value == 0
        t_dpar = timed(dev_parent)
        ok &= not bool(d_st.any().item())
        t_dacc = timed(dev_accept, lambda: seed(False))
        ok &= bool((d_state == M.ACC_NEW).all().item()) and not bool(d_st.any().item()) and dev_nm[0] == 0
        t_dhalf = timed(dev_accept, lambda: seed(True))
        ok &= bool((d_state[1::2] == M.ACC_KNOWN).all().item()) and dev_nm[0] == 0
        runs.append({"parent_ms": stat(t_par), "accept_ms": stat(t_acc), "half_known_ms": stat(t_half),
                     "dev_verify_ms": stat(t_dpar), "dev_accept_ms": stat(t_dacc), "dev_half_known_ms": stat(t_dhalf),
                     "index_ms": round(float(np.median(t_dacc) - np.median(t_dpar)), 3),
                     "host_accept_minus_parent_ms": round(float(np.median(t_acc) - np.median(t_par)), 3),
                     "index_entries": [s_acc.have, s_acc.wanted], "longest_probe": s_acc.longest_probe})
    mark("timed calls")
    stages = {"parent": staged(parent), "accept": staged(accept, lambda: seed(False)),
              "half_known": staged(accept, lambda: seed(True))}
    stages["dev_verify"] = staged(dev_parent)
    pipeline_ms = round(sum(stages["dev_verify"].values()), 3)
    print(json.dumps({"probe": "index", "blocks": n, "arena_bytes": total, "include_lookups": includes, "groups": int(grp[-1]) + 1,
                      "runs": runs, "stages_ms": stages, "pipeline_device_ms": pipeline_ms,
                      "index_below_pipeline": bool(all(r["index_ms"] < pipeline_ms for r in runs)),
                      "phase_s": {b[0]: round(b[1] - a_[1], 3) for a_, b in zip(stamps, stamps[1:])},
                      "results_ok": ok, "steps": a.steps, "warmup": a.warmup}))
    eng.host_free(arena)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
