"""What the indirect rule and the committed sequence cost: mv_commit_leaders beside mv_decide_leaders.

Input: tools/decide_probe.py's -- N config-4-shape blocks (100 authorities, 67 includes, one 512-B
Share, 66 VoteRanges), N / 100 rounds of one DAG -- in HBM, the genesis references seeded as
MV_REF_STORED, the DAG store reserved. The leader of round r is authority r mod 60, whose block every
block of round r + 1 includes, so every leader with two rounds above it commits directly. A second
DAG of the same shape thins the votes of every seventh leader: the 40 authors from 60 up leave its
block out (and take another in its place, so that every block keeps its quorum of includes): 60
votes, 40 blames, no certificate, so the direct rule leaves the row undecided and the indirect rule
skips it from the anchor three rounds up. Legs, each warmed up and then timed `--steps` times (the
median is reported), the whole measurement `--runs` times:

  a  whole_dag     the whole DAG connected in one call (not timed), then one commit call over one leader
                   per round, beside one decide call over the same rows
  b  thinned       the same on the thinned DAG: what the walks of 1 row in 7 add
  c  by_round      a round per mv_dev_connect_blocks call, each followed by a commit call over the rows
                   from the first one not yet in the sequence to the newest decidable round; against
                   the same delivery without the commit calls: the difference per call is the commit call

Every row of every commit call of legs a and b -- out, info and the sequence's length -- is compared
with tests/commit_seq_model.py's CommitRule before the probe prints its one JSON line; leg c's rows
are compared with leg a's / b's.

    python tools/commit_probe.py [--blocks N] [--steps K] [--warmup W] [--runs R]
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


def build_dag(engine, MB, rounds, n_auth, thin_every):
    """mysticeti_amd.blocks.build_rounds' config-4 shape; -> (bincodes, {reference: includes})."""
    prev = MB.genesis_refs(n_auth)
    seeds = np.frombuffer(b"".join(MB.authority_seed(a) for a in range(n_auth)), dtype=np.uint8).reshape(n_auth, 32)
    out, edges = [], {}
    for r in range(1, rounds + 1):
        thin = thin_every and r >= 2 and (r - 1) % thin_every == 0
        leader = (r - 1) % 60
        specs, msgs = [], []
        for a in range(n_auth):
            others = [x for x in range(n_auth) if x != a]
            inc = [prev[a]] + [prev[x] for x in others[:66]]
            if thin and a >= 60:
                spare = next(x for x in range(n_auth) if prev[x] not in inc)
                inc = [prev[spare] if i == prev[leader] else i for i in inc]
            ranges = [(prev[(a + 1 + v) % n_auth], 0, 1 + (v % 7)) for v in range(66)]
            t = r * 10**8 + a
            _, pre = MB.encode(a, r, inc, [MB.config4_tx(r, a)], ranges, t, 0, bytes(64), bytes(32))
            specs.append((a, inc, ranges, t, pre))
            msgs.append(MB._b2(pre))
        _, sig = engine.ed25519_sign(seeds, np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(-1, 32))
        cur = []
        for (a, inc, ranges, t, pre), s in zip(specs, sig):
            s = s.tobytes()
            d = MB._b2(pre + s)
            bn, _ = MB.encode(a, r, inc, [MB.config4_tx(r, a)], ranges, t, 0, s, d)
            out.append(bn)
            cur.append((a, r, d))
            edges[(a, r, d)] = inc
        prev = cur
    return out, edges


def model_rows(edges, n_auth, leaders):
    """CommitRule over the whole DAG. Its direct rule reads the records of rounds r .. r + 2 only, so
    each row's is given just those (every round here has records, so the lowest round is the same)."""
    import commit_model as C
    import commit_seq_model as S

    by_round = {}
    for ref, incs in edges.items():
        by_round.setdefault(ref[1], []).append((ref, incs))
    lowest = min(by_round)

    class Windowed(S.CommitRule):
        def decide(self, authority, rnd):
            if rnd < lowest:
                return C.DirectRule(self.stakes).decide(authority, rnd)
            d = C.DirectRule(self.stakes)
            d.records = [b for q in (rnd, rnd + 1, rnd + 2) for b in by_round.get(q, [])]
            assert by_round.get(rnd)
            return d.decide(authority, rnd)

    rule = Windowed([1] * n_auth)
    rule.records = [b for q in sorted(by_round) for b in by_round[q]]
    want, n_seq = rule.commit(leaders)
    return [w.row.words(a, r) for w, (a, r) in zip(want, leaders)], [w.info() for w in want], n_seq


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

    e = M.Engine(devices=(0,))
    n_auth, n = 100, a.blocks
    rounds = (n + n_auth - 1) // n_auth
    pks, stakes = MB.committee(e, n_auth, distinct=True)
    genesis = M.ref_words(MB.genesis_refs(n_auth))
    dev = torch.device("cuda", 0)
    t64 = lambda x: torch.from_numpy(x.view(np.int64).copy()).to(dev)
    slices = [(lo, min(lo + n_auth, n)) for lo in range(0, n, n_auth)]
    leaders = [(r % 60, r) for r in range(1, len(slices) + 1)]
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med = lambda v: float(np.median(v))

    def seed():
        e.index_clear()
        e.index_insert_stored(genesis)

    result, ok, reserved = {}, True, False
    for name, thin_every in (("whole_dag", 0), ("thinned", 7)):
        bins, edges = build_dag(e, MB, rounds, n_auth, thin_every)
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
        if not reserved:
            e.set_committee(pks, stakes, 0)
            e.index_reserve(n + includes + n_auth)
            e.pending_reserve(n, includes)
            e.dag_reserve(n, includes)
            reserved = True
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
        want_rows, want_info, want_seq = model_rows(edges, n_auth, leaders)
        got = {}

        def by_round(commit):
            rows, first, seq = 0, 0, []
            for k, (lo, hi) in enumerate(slices):
                m = hi - lo
                rows += e.dev_connect_blocks(0, d_arena, total, d_off_r[k, :m], d_len_r[k, :m], None, d_st_r[k, :m],
                                             d_state_r[k, :m], d_miss, d_rows_r[k, :m])[1]
                if commit and k >= 2 and first <= k - 2:  # rounds are k + 1: round k - 1 has its decision round now
                    c = e.commit_leaders(leaders[first:k - 1])
                    seq += c.rows[:c.n_sequence].tolist()
                    first += c.n_sequence
            got["rows"], got["seq"] = rows, seq

        runs = []
        for _ in range(a.runs):
            seed()
            _, nc = e.dev_connect_blocks(0, d_arena, total, d_off, d_len, d_grp, d_st, d_state, d_miss, d_rows)
            ok &= nc == n and e.dag_stats().records == n
            t_decide, t_commit = [], []
            for k in range(a.warmup + a.steps):  # interleaved
                t0 = time.perf_counter()
                dec = e.decide_leaders(leaders)
                t1 = time.perf_counter()
                com = e.commit_leaders(leaders)
                t2 = time.perf_counter()
                if k >= a.warmup:
                    t_decide.append((t1 - t0) * 1e3)
                    t_commit.append((t2 - t1) * 1e3)
            ok &= com.rows.tolist() == want_rows and com.info.tolist() == want_info and com.n_sequence == want_seq
            direct = [w if i[0] != 2 else [w[0], w[1], 0, 0, 0, 0, M.LEADER_UNDECIDED, w[7]] for w, i in zip(want_rows, want_info)]
            ok &= dec.rows.tolist() == direct
            run = {"decide_ms": stat(t_decide), "commit_ms": stat(t_commit),
                   "commit_minus_decide_ms": round(med(t_commit) - med(t_decide), 3)}
            t_plain, t_with = [], []
            for k in range(a.warmup + a.steps):  # interleaved
                for commit, ms in ((False, t_plain), (True, t_with)):
                    seed()
                    t0 = time.perf_counter()
                    by_round(commit)
                    if k >= a.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                    ok &= got["rows"] == n
            ok &= got["seq"] == want_rows[:want_seq]  # (no row of round 0 here)
            run.update({"connect_by_round_ms": stat(t_plain), "connect_commit_by_round_ms": stat(t_with),
                        "commit_added_per_call_ms": round((med(t_with) - med(t_plain)) / max(len(slices) - 2, 1), 4)})
            runs.append(run)
        kinds = [int(i[0]) for i in want_info]
        result[name] = {"rows": len(leaders), "direct": kinds.count(1), "indirect": kinds.count(2), "undecided": kinds.count(0),
                        "n_sequence": want_seq, "includes": includes, "runs": runs}
    print(json.dumps({"probe": "commit", "blocks": n, "rounds": len(slices), "legs": result, "results_ok": bool(ok),
                      "steps": a.steps, "warmup": a.warmup}))
    e.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
