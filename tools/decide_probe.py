"""What the DAG store and the direct decision rule cost: mv_decide_leaders beside mv_dev_connect_blocks.

Input: tools/connect_probe.py's -- N config-4-shape blocks (100 authorities, 67 includes, one 512-B
Share, 66 VoteRanges), N / 100 rounds of one DAG in delivery order -- in HBM, the genesis
references seeded as MV_REF_STORED. Two contexts read the same bytes: one with the DAG store
reserved (mv_dag_reserve), one without. The leader of round r is authority r mod 60, whose block
every block of round r + 1 includes, so every leader with two rounds above it commits. Legs, each
warmed up and then timed `--steps` times (the median is reported), the whole measurement `--runs`
times:

  a  whole_dag         the whole DAG connected in one call (not timed), then one decide call with one
                       leader per round: every row COMMIT but the last two rounds'
  b  by_round_decide   a round per mv_dev_connect_blocks call, each followed by a decide call for
                       the newest decidable round (r - 2); against the same delivery without the
                       decide calls on the same context: the difference per call is the decide call
  c  store on / off    the round-per-call delivery with and without the DAG store reserved: the
                       difference per call is the copy into the store

Between timed calls index and stores are cleared and seeded again (not timed). The probe checks its
own results before it prints one JSON line.

    python tools/decide_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
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

    plain, store = M.Engine(devices=(0,)), M.Engine(devices=(0,))
    n_auth, n = 100, a.blocks
    rounds = (n + n_auth - 1) // n_auth
    bins = MB.config4(plain, rounds=rounds)[:n]
    pks, stakes = MB.committee(plain, n_auth, distinct=True)
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
    own = [(int.from_bytes(b[0:8], "little"), int.from_bytes(b[8:16], "little"), bytes(b[24:56])) for b in bins]
    for e in (plain, store):
        e.set_committee(pks, stakes, 0)
        e.index_reserve(n + includes + n_auth)
        e.pending_reserve(n, includes)
    store.dag_reserve(n, includes)

    dev = torch.device("cuda", 0)
    d_arena = torch.from_numpy(arena).to(dev)
    t64 = lambda x: torch.from_numpy(x.view(np.int64).copy()).to(dev)
    d_off, d_len, d_grp = t64(offs), t64(lens), t64(grp)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_miss = torch.zeros((1024, 6), dtype=torch.int64, device=dev)
    d_rows = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    slices = [(lo, min(lo + n_auth, n)) for lo in range(0, n, n_auth)]
    d_st_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    d_state_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    pad64 = lambda x: np.concatenate([np.pad(x[lo:hi], (0, 128 - (hi - lo))) for lo, hi in slices]).astype(np.uint64)
    d_off_r, d_len_r = t64(pad64(offs)).view(len(slices), 128), t64(pad64(lens)).view(len(slices), 128)
    d_rows_r = torch.zeros((len(slices), 128, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    leaders = [(r % 60, r) for r in range(1, len(slices) + 1)]
    got = {}

    def seed(e):
        e.index_clear()
        e.index_insert_stored(genesis)

    def by_round(e, decide):
        rows, statuses = 0, []
        for k, (lo, hi) in enumerate(slices):
            m = hi - lo
            rows += e.dev_connect_blocks(0, d_arena, total, d_off_r[k, :m], d_len_r[k, :m], None, d_st_r[k, :m],
                                         d_state_r[k, :m], d_miss, d_rows_r[k, :m])[1]
            if decide and k >= 2:  # rounds are k + 1: round k - 1 has its decision round now
                statuses.append(int(e.decide_leaders([leaders[k - 2]]).rows[0, 6]))
        got["rows"], got["statuses"] = rows, statuses

    def timed(e, fn):
        ms = []
        for k in range(a.warmup + a.steps):
            seed(e)
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med = lambda v: float(np.median(v))
    full = len(slices) if n % n_auth == 0 else len(slices) - 1  # whole rounds
    runs, ok = [], True
    for _ in range(a.runs):
        # a: the whole DAG, one decide call
        seed(store)
        nm, nc = store.dev_connect_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss, d_rows)
        ok &= nc == n and store.dag_stats().records == n
        t_whole = []
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            dec = store.decide_leaders(leaders)
            if k >= a.warmup:
                t_whole.append((time.perf_counter() - t0) * 1e3)
        want = [M.LEADER_COMMIT] * max(full - 2, 0)
        ok &= dec.status.tolist()[:len(want)] == want and dec.status.tolist()[-2:] == [M.LEADER_UNDECIDED] * 2
        ok &= all(dec.ref(i) == own[n_auth * i + leaders[i][0]] for i in range(len(want)))
        # b, c: a round per call
        t_plain = timed(plain, lambda: by_round(plain, False))
        ok &= got["rows"] == n
        t_store = timed(store, lambda: by_round(store, False))
        ok &= got["rows"] == n and store.dag_stats().records == n
        t_decide = timed(store, lambda: by_round(store, True))
        ok &= got["rows"] == n and got["statuses"][:max(full - 2, 0)] == want
        calls = len(slices)
        runs.append({"decide_whole_dag_ms": stat(t_whole), "connect_by_round_ms": stat(t_plain),
                     "connect_by_round_store_ms": stat(t_store), "connect_decide_by_round_ms": stat(t_decide),
                     "connect_per_call_ms": round(med(t_plain) / calls, 4),
                     "store_added_per_call_ms": round((med(t_store) - med(t_plain)) / calls, 4),
                     "decide_added_per_call_ms": round((med(t_decide) - med(t_store)) / max(calls - 2, 1), 4)})
    print(json.dumps({"probe": "decide", "blocks": n, "includes": includes, "rounds": len(slices), "runs": runs,
                      "results_ok": bool(ok), "steps": a.steps, "warmup": a.warmup}))
    plain.close()
    store.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
