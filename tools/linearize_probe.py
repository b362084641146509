"""What the linearizer costs: mv_linearize behind mv_commit_leaders.

Input: tools/commit_probe.py's whole DAG -- N config-4-shape blocks (100 authorities, 67 includes, one
512-B Share, 66 VoteRanges), N / 100 rounds -- in HBM, the genesis references seeded as MV_REF_STORED,
the DAG store reserved. Every leader with two rounds above it commits directly; the committed
references of the sequence are what mv_linearize is given. Legs, each warmed up and then timed
`--steps` times (the median is reported), the whole measurement `--runs` times:

  a  whole_sequence  the whole DAG connected in one call and one commit call (neither timed), then the
                     whole committed sequence in one linearize call; before each step the index is
                     cleared and the DAG connected again (not timed), which empties the marks
  b  by_round        a round per mv_dev_connect_blocks call, each followed by a commit call and a
                     linearize call over the leaders that call committed; against the same delivery
                     with the commit calls alone: the difference per call is the linearize call
  c  verbatim        tests/linearize_model.py's Verbatim (the reference's stack loop) in Python over
                     the same sequence, for scale only

Every sub row and every block row of legs a and b is compared with tests/linearize_model.py's
LevelRule, and LevelRule's blocks with Verbatim's, before the probe prints its one JSON line. The
launch count of leg a is computed from the call's shape as engine_linearize.cpp lays it out: roots, two
edge walks, per level five pick launches and one take (one pick and one take for a level no edge
ends in), rows, out.

    python tools/linearize_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import linearize_model as L
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB
    from commit_probe import build_dag

    e = M.Engine(devices=(0,))
    n_auth, n = 100, a.blocks
    rounds = (n + n_auth - 1) // n_auth
    pks, stakes = MB.committee(e, n_auth, distinct=True)
    genesis_refs = MB.genesis_refs(n_auth)
    genesis = M.ref_words(genesis_refs)
    dev = torch.device("cuda", 0)
    t64 = lambda x: torch.from_numpy(x.view(np.int64).copy()).to(dev)
    slices = [(lo, min(lo + n_auth, n)) for lo in range(0, n, n_auth)]
    leaders = [(r % 60, r) for r in range(1, len(slices) + 1)]
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med = lambda v: float(np.median(v))

    def seed():
        e.index_clear()
        e.index_insert_stored(genesis)

    bins, edges = build_dag(e, MB, rounds, n_auth, 0)
    bins = bins[:n]
    edges = {ref: inc for ref, inc in list(edges.items())[:n]}
    lens = np.array([len(b) for b in bins], dtype=np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum((lens + np.uint64(7)) & ~np.uint64(7))[:-1]
    total = int(offs[-1] + lens[-1])
    arena = np.zeros(total + 64, dtype=np.uint8)
    for o, b in zip(offs.tolist(), bins):
        arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    includes = sum(len(v) for v in edges.values())
    e.set_committee(pks, stakes, 0)
    e.index_reserve(n + includes + n_auth)
    e.pending_reserve(n, includes)
    e.dag_reserve(n, includes)
    d_arena = torch.from_numpy(arena).to(dev)
    grp = (np.arange(n, dtype=np.uint64) // np.uint64(n_auth)).astype(np.uint64)
    d_off, d_len, d_grp = t64(offs), t64(lens), t64(grp)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_miss = torch.zeros((1024, 6), dtype=torch.int64, device=dev)
    d_rows = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    pad64 = lambda x: np.concatenate([np.pad(x[lo:hi], (0, 128 - (hi - lo))) for lo, hi in slices]).astype(np.uint64)
    d_off_r, d_len_r = t64(pad64(offs)).view(len(slices), 128), t64(pad64(lens)).view(len(slices), 128)
    d_st_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    d_state_r = torch.zeros((len(slices), 128), dtype=torch.uint8, device=dev)
    d_rows_r = torch.zeros((len(slices), 128, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    cap = n + n_auth + 16
    ok, got = True, {}

    def committed(c):
        """The references of the COMMIT rows of a commit call's sequence, (k, 6) uint64."""
        seq = c.rows[[i for i, _ in c.sequence()]] if c.n_sequence else c.rows[:0]
        return np.ascontiguousarray(seq[seq[:, 6] == M.LEADER_COMMIT][:, :6])

    def as_refs(rows):
        return [(int(r[0]), int(r[1]), r[2:].astype("<u8").tobytes()) for r in rows]

    def by_round(commit, linear):
        rows, first, blocks, subs = 0, 0, [], []
        for k, (lo, hi) in enumerate(slices):
            m = hi - lo
            rows += e.dev_connect_blocks(0, d_arena, total, d_off_r[k, :m], d_len_r[k, :m], None, d_st_r[k, :m],
                                         d_state_r[k, :m], d_miss, d_rows_r[k, :m])[1]
            if commit and k >= 2 and first <= k - 2:
                c = e.commit_leaders(leaders[first:k - 1])
                first += c.n_sequence
                if linear:
                    lin = e.linearize(committed(c), 4096)
                    blocks.append(lin.blocks)
                    subs += lin.sub[:, [0, 2]].tolist()
        got["rows"], got["blocks"], got["subs"] = rows, blocks, subs

    # the model's answer: LevelRule over the whole DAG, and Verbatim beside it
    seed()
    _, nc = e.dev_connect_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss, d_rows)
    ok &= nc == n and e.dag_stats().records == n
    seq_refs = committed(e.commit_leaders(leaders))
    lead = as_refs(seq_refs)
    want_blocks, want_sub = L.LevelRule(edges).linearize(lead, cap)
    want_words = M.ref_words(want_blocks)
    ok &= all(r[0] == L.OK for r in want_sub) and len(lead) > 0
    everything = dict(edges)
    everything.update({g: [] for g in genesis_refs})
    t_verbatim = []
    for _ in range(2):
        v = L.Verbatim(everything)
        t0 = time.perf_counter()
        out = v.handle_commit(lead)
        t_verbatim.append((time.perf_counter() - t0) * 1e3)
    ok &= [b for blocks, _ in out for b in blocks] == want_blocks

    # leg a's launch count, from the call's shape
    hi = max(x[1] for x in lead)
    ends = {i[1] for ref, inc in edges.items() if ref[1] <= hi for i in inc}
    stands = {x[1] for x in lead}
    levels = sorted(ends | stands)
    launches = 3 + sum(6 if q in ends else 2 for q in levels) + 2

    runs = []
    for _ in range(a.runs):
        t_lin = []
        for k in range(a.warmup + a.steps):
            seed()  # empties the marks (and the store: connect again, not timed)
            _, nc = e.dev_connect_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss, d_rows)
            ok &= nc == n
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            lin = e.linearize(seq_refs, cap)
            t1 = time.perf_counter()
            if k >= a.warmup:
                t_lin.append((t1 - t0) * 1e3)
            ok &= lin.sub.tolist() == want_sub and np.array_equal(lin.blocks, want_words)
            st = e.linearize_stats()
            ok &= (st.marked, st.last_height) == (len(want_blocks), len(lead))
        run = {"linearize_whole_sequence_ms": stat(t_lin)}
        t_plain, t_commit, t_both = [], [], []
        for k in range(a.warmup + a.steps):  # interleaved
            for commit, linear, ms in ((False, False, t_plain), (True, False, t_commit), (True, True, t_both)):
                seed()
                t0 = time.perf_counter()
                by_round(commit, linear)
                if k >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
                ok &= got["rows"] == n
        ok &= np.array_equal(np.concatenate(got["blocks"]), want_words)
        ok &= got["subs"] == [[r[0], r[2]] for r in want_sub]
        calls = max(len(slices) - 2, 1)
        run.update({"connect_by_round_ms": stat(t_plain), "connect_commit_by_round_ms": stat(t_commit),
                    "connect_commit_linearize_by_round_ms": stat(t_both),
                    "commit_added_per_call_ms": round((med(t_commit) - med(t_plain)) / calls, 4),
                    "linearize_added_per_call_ms": round((med(t_both) - med(t_commit)) / calls, 4)})
        runs.append(run)
    result = {"leaders": len(lead), "blocks_out": len(want_blocks), "includes": includes,
              "levels": len(levels), "launches_per_level": 6, "launches_whole_sequence": launches,
              "index_slots_key_bytes": 40, "verbatim_python_ms": stat(t_verbatim), "runs": runs}
    print(json.dumps({"probe": "linearize", "blocks": n, "rounds": len(slices), "legs": result, "results_ok": bool(ok),
                      "steps": a.steps, "warmup": a.warmup}))
    e.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
