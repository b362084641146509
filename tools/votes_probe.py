"""What vote aggregation costs: mv_aggregate_votes on the config-4 DAG shape.

Input: N blocks of the config-4 shape (100 authorities, one 512-byte Share, 66 VoteRanges over
blocks of the round before), N / 100 rounds, unsigned: the call does not verify.
Legs, each warmed up `--warmup` times and then timed `--steps` times (the median is reported), the
whole measurement `--runs` times:

  a  whole_dag   the whole DAG in one call (host buffers: copy in, the call, copy out)
  b  by_round    a round per call
  c  cell_rule   the same through tests/votes_model.py's CellRule in Python, once, for scale only

Before anything is printed every output of legs a and b -- per-block status and counts, the
certified rows and their order, the statistics -- is compared with CellRule. Writes
profiles/votes/votes_probe.json and prints it as one line.

    python tools/votes_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_AUTH, N_VR = 100, 66


def build_dag(vc, rounds):
    prev, out = None, []
    for r in range(1, rounds + 1):
        cur = []
        for a in range(N_AUTH):
            sts = [("share", bytes([r & 255, a]) * 256)]
            if prev:
                sts += [("range", prev[(a + 1 + v) % N_AUTH][1], 0, 1 + (v % 7)) for v in range(N_VR)]
            else:
                sts += [("range", vc.ref_of((a + 1 + v) % N_AUTH, 0, "genesis"), 0, 1 + (v % 7)) for v in range(N_VR)]
            cur.append(vc.block(a, r, sts))
        out += cur
        prev = cur
    return out


def expected(vc, CellRule, stakes, blocks, cuts):
    model, calls = CellRule(stakes), []
    t0 = time.perf_counter()
    for lo, hi in zip(cuts, cuts[1:]):
        counts, rows = [], []
        for i, b in enumerate(blocks[lo:hi]):
            r = model.process_block(b)
            counts.append([len(r.processed), r.unknown, r.duplicate, r.flags])
            rows += [list(vc.ref_words(ref)) + [o, i] for ref, o in r.processed]
        calls.append((counts, rows))
    return calls, (model.len(), model.aggregating(), model.certified), time.perf_counter() - t0


def run_leg(e, bins, cuts, want, want_stats, check):
    e.votes_clear()
    e.votes_reserve(len(bins), 2 * len(bins))
    t0 = time.perf_counter()
    got = [e.aggregate_votes(bins[lo:hi], cap_certified=len(w[1]) + 1) for (lo, hi), w in zip(zip(cuts, cuts[1:]), want)]
    dt = time.perf_counter() - t0
    if check:
        for (st, counts, rows, total), (wc, wr) in zip(got, want):
            assert not st.any() and counts.tolist() == wc and total == len(wr) and rows.tolist() == wr
        s = e.votes_stats()
        assert (s.pending, s.aggregating, s.certified) == want_stats, (s.as_tuple(), want_stats)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    import mysticeti_amd as M
    import votes_cases as vc
    from mysticeti_amd import blocks as MB
    from votes_model import CellRule

    rounds = max(2, a.blocks // N_AUTH)
    blocks = build_dag(vc, rounds)
    bins = [vc.encode_block(b) for b in blocks]
    stakes = [1] * N_AUTH
    legs = {"whole_dag": [0, len(blocks)], "by_round": list(range(0, len(blocks) + 1, N_AUTH))}
    out = {"blocks": len(blocks), "authorities": N_AUTH, "vote_ranges": N_VR, "steps": a.steps, "warmup": a.warmup,
           "runs": []}
    with M.Engine(devices=(0,)) as e:
        pk = MB.committee(e, 1, False)[0][0]
        e.set_committee(np.tile(pk, (N_AUTH, 1)), np.asarray(stakes, dtype=np.uint64))
        want = {}
        for name, cuts in legs.items():
            want[name] = expected(vc, CellRule, stakes, blocks, cuts)
        out["cell_rule_python_s"] = want["whole_dag"][2]
        out["certified"] = want["whole_dag"][1][2]
        for _ in range(a.runs):
            run = {}
            for name, cuts in legs.items():
                calls, stats, _ = want[name]
                for k in range(a.warmup):
                    run_leg(e, bins, cuts, calls, stats, check=True)
                ts = [run_leg(e, bins, cuts, calls, stats, check=False) for _ in range(a.steps)]
                run[name + "_ms"] = 1e3 * statistics.median(ts)
                run[name + "_blocks_per_s"] = len(blocks) / statistics.median(ts)
            out["runs"].append(run)
    out["self_check"] = "passed"
    os.makedirs(os.path.join(ROOT, "profiles", "votes"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "votes", "votes_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
