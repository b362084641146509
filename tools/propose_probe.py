"""What proposing costs: mv_propose_add and mv_propose_take with one full round pending.

Cases: committees of 100 and of 512 equal seats. The DAG is two full rounds (every block includes
every block of the round before). Before the timed calls, not timed: the index is cleared, genesis
seeded, the state reserved for seat 0, the genesis loop and the own genesis block put in, all blocks
connected, round 1 added, taken and confirmed with an own block of round 2. What is timed, per step:

  add    one mv_propose_add over the n connected rows of round 2 and n seeded references of round 3
         (they move the clock past round 2), 2 n rows of two rounds: resolve, one sort pass, append,
         the segment scan and the chain. `add_ms` is host wall clock around the synchronous call;
         `dev_add_event_ms` is the same call's device-buffer variant on a stream of the probe's own,
         bracketed by two events on that stream (the span on the device, its idle gaps included).
  take   one mv_propose_take: the queue holds the 2 n entries, all are taken; the n round-2 records are
         stamped (n x n includes) with the own last block's, the 2 n entries are compacted. Host wall
         clock around the synchronous call.
  host   the same choice by tools/propose_host.cpp: std::unordered_set over six-word references on one
         host core (the reference's HashSet, core.rs:254-271), timed inside the helper.

Each leg is warmed up and then run `--steps` times; the median, the least and the largest are
reported. The includes of every timed take are compared with the helper's and with
tests/propose_model.py's Core before the probe prints its one JSON line (also written to
profiles/propose/propose_probe.json). With --host-only the GPU legs are left out (no GPU needed):
the DAG's references are made up instead of signed blocks.

    python tools/propose_probe.py [--seats 100,512] [--steps K] [--warmup W] [--host-only]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # (what the tests' helpers import)
HELPER_SRC = os.path.join(ROOT, "tools", "propose_host.cpp")
HELPER = os.path.join(ROOT, "tools", "libpropose_host.so")
OUT = os.path.join(ROOT, "profiles", "propose", "propose_probe.json")


def helper():
    if not os.path.exists(HELPER) or os.path.getmtime(HELPER) < os.path.getmtime(HELPER_SRC):
        subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-o", HELPER, HELPER_SRC],
                       check=True)
    lib = ctypes.CDLL(HELPER)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.propose_host_choice.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp]
    lib.propose_host_choice.restype = u64
    return lib


def host_choice(lib, own, taken, incs):
    """(kept (k, 6) words, ms): own (m, 6), taken (t, 6), incs: per taken block its (k_i, 6) includes."""
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    off = np.zeros(len(incs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(i) for i in incs])
    flat = np.ascontiguousarray(np.concatenate([i for i in incs if len(i)] or [np.zeros((0, 6), dtype=np.uint64)]))
    flat = flat if len(flat) else np.zeros((1, 6), dtype=np.uint64)
    n_own = len(own)
    own = np.ascontiguousarray(own) if n_own else np.zeros((1, 6), dtype=np.uint64)
    out = np.zeros((max(len(taken), 1), 6), dtype=np.uint64)
    ns = ctypes.c_uint64(0)
    k = lib.propose_host_choice(p(own), n_own, p(taken), len(taken), p(flat), p(off), p(out), ctypes.byref(ns))
    return out[:k], ns.value / 1e6


def stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def made_up(n):
    """References of a two-round full DAG without blocks (for --host-only)."""
    ref = lambda a, r: (a, r, (a * 1_000_003 + r).to_bytes(8, "little") * 4)
    g = [ref(a, 0) for a in range(n)]
    r1 = [ref(a, 1) for a in range(n)]
    r2 = [ref(a, 2) for a in range(n)]
    return g, r1, r2


def case(n, a, lib, e):
    import mysticeti_amd as M
    import propose_model as PM

    r3 = [(s, 3, bytes([7]) + bytes(31)) for s in range(n)]
    own2 = (0, 2, bytes([9]) + bytes(31))
    if e is None:
        g, r1, r2 = made_up(n)
        blocks = {r: list(g) for r in r1}
        blocks.update({r: list(r1) for r in r2})
        bins = None
    else:
        from test_gpu_decide import Dag

        d = Dag(e, n, [1] * n, distinct=False)
        g, r1, r2 = d.genesis, d.full(), d.full()
        blocks = {r: list(i) for r, (_, i) in d.blocks.items()}
        bins = d.bins
        e.set_committee(d.pks, np.ones(n, dtype=np.uint64), 0)
    W = M.ref_words
    # the model's answer, and the helper's on the same sets
    m = PM.Core([1] * n, 0)
    m.blocks = dict(blocks)
    m.add_blocks(g[1:], in_order=True)
    m.own_block(g[0], [])
    m.add_blocks(r1)
    m.try_new_block()
    m.own_block(own2)
    own_inc = list(m.own[1])
    m.add_blocks(r2 + r3)
    _, want, _, taken, _, _ = m.try_new_block()
    ok = taken == 2 * n
    t_words = W(r2 + r3)
    inc_words = [W(blocks[r]) for r in r2] + [np.zeros((0, 6), dtype=np.uint64)] * n
    t_host = []
    for k in range(a.warmup + a.steps):
        kept, ms = host_choice(lib, W(own_inc), t_words, inc_words)
        if k >= a.warmup:
            t_host.append(ms)
    ok &= np.array_equal(kept, W(want))
    res = {"seats": n, "rows_per_add": 2 * n, "entries_taken": 2 * n, "set_inserts": n * n + len(own_inc),
           "includes_kept": len(want), "host_unordered_set_ms": stat(t_host)}
    if e is None:
        return res, ok
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    t_add, t_take, t_dev = [], [], []

    def before():
        e.index_clear()
        e.index_insert_stored(g)
        e.index_insert_stored(r3)
        e.propose_reserve(0, 4 * n)
        e.propose_add(g[1:], in_order=True)
        e.propose_own(g[0], [])
        c = e.connect_blocks(bins)
        rows = c.connected
        first = rows[rows[:, 1] == 1]
        e.propose_add(first)
        e.propose_take(2 * n, 8)
        e.propose_own(own2)
        second = np.zeros((2 * n, 8), dtype=np.uint64)
        second[:n] = rows[rows[:, 1] == 2]
        second[n:, :6] = W(r3)
        return c.n_connected == 2 * n, second

    for k in range(a.warmup + a.steps):
        good, second = before()
        ok &= good
        t0 = time.perf_counter()
        e.propose_add(second, tags=np.arange(2 * n, dtype=np.uint64))
        t1 = time.perf_counter()
        t = e.propose_take(4 * n, 8)
        t2 = time.perf_counter()
        ok &= t.proposed == 1 and np.array_equal(t.includes, W(want)) and t.guard_intact
        if k >= a.warmup:
            t_add.append((t1 - t0) * 1e3)
            t_take.append((t2 - t1) * 1e3)
        # the device-buffer add, bracketed by events on the probe's stream
        good, second = before()
        ok &= good
        d_rows = torch.from_numpy(second.view(np.int64)).to(dev)
        torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        clock = e.dev_propose_add(0, d_rows, None, stream_handle=stream.cuda_stream)
        ev1.record(stream)
        ev1.synchronize()
        ok &= clock.round == 4
        if k >= a.warmup:
            t_dev.append(ev0.elapsed_time(ev1))
    res.update({"add_ms": stat(t_add), "take_ms": stat(t_take), "dev_add_event_ms": stat(t_dev)})
    return res, ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seats", default="100,512")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    lib = helper()
    e = None
    if not a.host_only:
        import torch

        torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
        import mysticeti_amd as M

        e = M.Engine(devices=(0,))
        e.dag_reserve(2048, 1 << 20)
    cases, ok = [], True
    for n in (int(x) for x in a.seats.split(",")):
        res, good = case(n, a, lib, e)
        cases.append(res)
        ok &= bool(good)
    if e is not None:
        e.close()
    line = json.dumps({"probe": "propose", "host_only": a.host_only, "steps": a.steps, "warmup": a.warmup,
                       "timing": "add_ms, take_ms: host wall clock around the synchronous call; dev_add_event_ms: "
                                 "events on the caller's stream; host_unordered_set_ms: inside the helper",
                       "cases": cases, "results_ok": bool(ok)})
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    out = OUT if not a.host_only else OUT.replace(".json", "_host.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
