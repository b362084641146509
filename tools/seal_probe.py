"""What building a signed DAG costs with and without mv_seal_blocks.

  a  the builder as it stands: blocks.config4(engine, rounds) -- per round the host encodes, hashes
     every pre-image, signs the round in one GPU call, hashes pre-image || signature, splices the
     digests into the next round. Wall time per DAG and per round.
  b  blocks.build_rounds_sealed on the same shape: every round encoded once with placeholders, one
     linked seal call. Wall time per DAG, and of the seal call alone per DAG and per level; and the
     same linked call on the DAG resident in HBM (mv_dev_seal_blocks: no copy of the blocks either
     way), per DAG and per level -- a level's device step with its launch.
  c  one unlinked mv_dev_seal_blocks call over 2^17 independent config-4-shape blocks resident in
     HBM, in blocks/s, next to mv_dev_verify_blocks over the same buffer.

Each leg: `--warmup` runs, then the median of `--steps`; the whole measurement `--runs` times.
Before anything is printed, b's first two rounds are held against tests/seal_model.py and all its
blocks against mv_verify_blocks, and c's sealed image against the builder's bytes. Writes
profiles/seal/seal_probe.json and prints it as one JSON line.

    python tools/seal_probe.py [--rounds R] [--blocks N] [--steps K] [--warmup W] [--runs 2]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the model


def median_of(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=328)
    ap.add_argument("--blocks", type=int, default=1 << 17)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seal", "seal_probe.json"))
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB
    import seal_model as S

    eng = M.Engine(devices=(0,))
    n_auth = 100
    seeds = [MB.authority_seed(x) for x in range(n_auth)]
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)

    # correctness first
    sealed = MB.build_rounds_sealed(eng, a.rounds, n_auth, seeds, 67, 66, True)
    st, _, _ = eng.verify_blocks(sealed)
    assert not st.any(), "a sealed block does not verify"
    head = sealed[:2 * n_auth]
    want, o, l = S.pack(S.unseal(head))
    assert S.seal(want, o, l, seeds, link=True)[0] == [S.OK] * len(head)
    assert bytes(want[:o[-1] + l[-1]]) == b"".join(head), "the sealed DAG is not the model's"

    dev = torch.device("cuda", 0)
    dag = np.frombuffer(b"".join(sealed) + bytes(16), dtype=np.uint8).copy()
    g_len = np.array([len(b) for b in sealed], dtype=np.int64)
    g_off = np.zeros(len(sealed), dtype=np.int64)
    g_off[1:] = np.cumsum(g_len)[:-1]
    g_buf, g_offd, g_lend = torch.from_numpy(dag).to(dev), torch.from_numpy(g_off).to(dev), torch.from_numpy(g_len).to(dev)
    g_st = torch.zeros(len(sealed), dtype=torch.uint8, device=dev)

    base = MB.config4(eng, 41)  # 4,100 distinct blocks, repeated
    n = a.blocks
    lens = np.array([len(base[i % len(base)]) for i in range(n)], dtype=np.int64)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum(lens)[:-1]
    one = np.frombuffer(b"".join(base), dtype=np.uint8)
    total = int(lens.sum())
    image = np.zeros(total + 16, dtype=np.uint8)
    for k in range(0, n, len(base)):
        m = min(len(base), n - k)
        image[offs[k]:offs[k] + int(lens[k:k + m].sum())] = one[:int(lens[k:k + m].sum())]
    blank = image.copy()
    for i in range(n):  # own digest and signature (the bincode's last 64 bytes) zeroed
        blank[offs[i] + 24:offs[i] + 56] = 0
        blank[offs[i] + lens[i] - 64:offs[i] + lens[i]] = 0
    d_buf = torch.from_numpy(blank).to(dev)
    d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    d_seeds = torch.from_numpy(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_auth, 32).copy()).to(dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_md = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_bd = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_seal_blocks(0, d_buf, total, d_off, d_len, d_seeds, d_st, d_md, d_bd)
    assert not d_st.any().item() and np.array_equal(d_buf.cpu().numpy(), image), "the sealed image is not the builder's"

    def dev_linked():  # sealing a sealed DAG again writes the same bytes: every repeat does the whole work
        eng.dev_seal_blocks(0, g_buf, len(dag) - 16, g_offd, g_lend, d_seeds, g_st, link=True)

    dev_linked()
    assert not g_st.any().item() and np.array_equal(g_buf.cpu().numpy(), dag), "the re-sealed DAG changed"

    def verify():
        eng.dev_verify_blocks(0, d_buf, total, d_off, d_len, d_st, d_md, d_bd)
        torch.cuda.synchronize()

    verify()
    assert not d_st.any().item()

    seal_s = []
    inner = eng.seal_blocks

    def timed_seal(*args, **kw):
        t0 = time.perf_counter()
        r = inner(*args, **kw)
        seal_s.append(time.perf_counter() - t0)
        return r

    runs = []
    for _ in range(a.runs):
        ta = median_of(lambda: MB.config4(eng, a.rounds), a.warmup, a.steps)
        eng.seal_blocks = timed_seal
        seal_s.clear()
        tb = median_of(lambda: MB.build_rounds_sealed(eng, a.rounds, n_auth, seeds, 67, 66, True), a.warmup, a.steps)
        del eng.seal_blocks
        tcall = statistics.median(seal_s[a.warmup:])
        tg = median_of(dev_linked, a.warmup, a.steps)
        tc = median_of(lambda: eng.dev_seal_blocks(0, d_buf, total, d_off, d_len, d_seeds, d_st, d_md, d_bd), a.warmup, a.steps)
        tv = median_of(verify, a.warmup, a.steps)
        runs.append({
            "a_builder_s_per_dag": ta, "a_builder_ms_per_round": 1e3 * ta / a.rounds,
            "b_sealed_s_per_dag": tb, "b_seal_call_s_per_dag": tcall, "b_seal_call_ms_per_level": 1e3 * tcall / a.rounds,
            "b_dev_linked_s_per_dag": tg, "b_dev_linked_ms_per_level": 1e3 * tg / a.rounds,
            "b_over_a_speedup": ta / tb,
            "c_seal_blocks_per_s": n / tc, "c_verify_blocks_per_s": n / tv,
        })
    out = {"probe": "seal", "rounds": a.rounds, "dag_blocks": a.rounds * n_auth, "c_blocks": n, "c_bytes": total,
           "steps": a.steps, "warmup": a.warmup, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
