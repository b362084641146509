"""What the connect sweep costs: mv_dev_connect_blocks against mv_dev_accept_blocks on one arena.

Input: tools/index_probe.py's -- N config-4-shape blocks (100 authorities, 67 includes, one 512-B
Share, 66 VoteRanges), N / 100 rounds of one DAG in delivery order -- in HBM, the genesis
references seeded as MV_REF_STORED. Every block includes 67 blocks of the round before, so round r
connects at level r - 1. Three legs in device-buffer calls over the same bytes, each warmed up and
then timed `--steps` times (the median is reported), the whole measurement `--runs` times:

  accept      mv_dev_accept_blocks on the whole arena: the parent's call, unchanged in this tree
  by_round    mv_dev_connect_blocks delivered one round per call: every call appends 100 blocks
              and releases them at level 0 (the sum over the rounds is reported, and the same
              delivery through mv_dev_accept_blocks beside it: the sweep is the difference)
  one_call    the whole DAG in one call: N / 100 levels over a store of N blocks

Between timed calls the index is cleared and seeded again (not timed). Prints one JSON line.

    python tools/connect_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
"""
import argparse
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
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    eng = M.Engine(devices=(0,))
    n_auth, n = 100, a.blocks
    rounds = (n + n_auth - 1) // n_auth
    bins = MB.config4(eng, rounds=rounds)[:n]
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum((lens + np.uint64(7)) & ~np.uint64(7))[:-1]
    total = int(offs[-1] + lens[-1])
    arena = np.zeros(total + 64, dtype=np.uint8)
    for o, b in zip(offs.tolist(), bins):
        arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    grp = (np.arange(n, dtype=np.uint64) // np.uint64(n_auth)).astype(np.uint64)
    includes = int(sum(int.from_bytes(b[56:64], "little") for b in bins))
    genesis = M.ref_words(MB.genesis_refs(n_auth))
    eng.index_reserve(n + includes + n_auth)  # a device-buffer call asks for room for every include it may add
    eng.pending_reserve(n, includes)

    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(arena).to(dev)
    t64 = lambda x: torch.from_numpy(x.view(np.int64).copy()).to(dev)
    d_off, d_len, d_grp = t64(offs), t64(lens), t64(grp)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_miss = torch.zeros((1024, 6), dtype=torch.int64, device=dev)
    d_rows = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    slices = [(lo, min(lo + n_auth, n)) for lo in range(0, n, n_auth)]
    # per-round outputs at a 128-byte stride, and offsets / lengths of their own: every pointer a
    # device-buffer call gets is 16-byte aligned
    d_st_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    d_state_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    pad64 = lambda x: np.concatenate([np.pad(x[lo:hi], (0, 128 - (hi - lo))) for lo, hi in slices]).astype(np.uint64)
    d_off_r, d_len_r = t64(pad64(offs)).view(len(slices), 128), t64(pad64(lens)).view(len(slices), 128)
    d_rows_r = torch.zeros((len(slices), 128, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    got = {}

    def seed():
        eng.index_clear()
        eng.index_insert_stored(genesis)

    def accept():
        got["missing"] = eng.dev_accept_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss)

    def accept_by_round():
        for k, (lo, hi) in enumerate(slices):
            m = hi - lo
            eng.dev_accept_blocks(0, d_arena, total, d_off_r[k, :m], d_len_r[k, :m], None, d_st_r[k, :m], d_state_r[k, :m], d_miss)

    def by_round():
        rows = 0
        for k, (lo, hi) in enumerate(slices):
            m = hi - lo
            rows += eng.dev_connect_blocks(0, d_arena, total, d_off_r[k, :m], d_len_r[k, :m], None, d_st_r[k, :m],
                                           d_state_r[k, :m], d_miss, d_rows_r[k, :m])[1]
        got["rows"] = rows

    def one_call():
        got["missing"], got["rows"] = eng.dev_connect_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state,
                                                            d_miss, d_rows)

    def timed(fn):
        ms = []
        for k in range(a.warmup + a.steps):
            seed()
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    all_new = lambda: bool((d_state == M.ACC_NEW).all().item()) and not bool(d_st.any().item())
    counts = torch.tensor([hi - lo for lo, hi in slices], device=dev)
    live = torch.arange(128, device=dev)[None, :] < counts[:, None]  # the entries of the per-round outputs in use

    def all_new_r():
        return bool((d_state_r[live] == M.ACC_NEW).all().item()) and not bool(d_st_r[live].any().item())

    def clear_r():
        d_state_r.zero_()
        d_st_r.fill_(1)

    runs, ok = [], True
    for _ in range(a.runs):
        t_acc = timed(accept)
        ok &= all_new() and got["missing"] == 0
        clear_r()
        t_accr = timed(accept_by_round)
        ok &= all_new_r()
        clear_r()
        t_round = timed(by_round)
        ps = eng.pending_stats()
        ok &= all_new_r() and got["rows"] == n and (ps.stored, ps.suspended, ps.levels) == (n + n_auth, 0, 1)
        t_one = timed(one_call)
        ps = eng.pending_stats()
        rows = d_rows.cpu().numpy().view(np.uint64)
        ok &= all_new() and got["rows"] == n and (ps.stored, ps.suspended, ps.levels) == (n + n_auth, 0, len(slices))
        ok &= bool((rows[:, 7] == rows[:, 1] - np.uint64(1)).all()) and bool((np.diff(rows[:, 7].astype(np.int64)) >= 0).all())
        sweep_one = float(np.median(t_one) - np.median(t_acc))
        runs.append({"accept_ms": stat(t_acc), "accept_by_round_ms": stat(t_accr), "connect_by_round_ms": stat(t_round),
                     "connect_one_call_ms": stat(t_one),
                     "sweep_by_round_ms": round(float(np.median(t_round) - np.median(t_accr)), 3),
                     "sweep_by_round_per_call_ms": round(float(np.median(t_round) - np.median(t_accr)) / len(slices), 4),
                     "sweep_one_call_ms": round(sweep_one, 3),
                     "one_call_per_level_ms": round(sweep_one / len(slices), 4)})
    print(json.dumps({"probe": "connect", "blocks": n, "arena_bytes": total, "includes": includes, "levels": len(slices),
                      "runs": runs, "results_ok": ok, "steps": a.steps, "warmup": a.warmup}))
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
