"""What building a signed DAG costs with the host encode and with mv_encode_blocks.

  a  blocks.build_rounds_sealed per DAG: the host encodes every block with placeholders, one linked
     seal call. This library's seal is launch for launch the one that path always used.
  b  blocks.build_rounds_encoded per DAG: the numpy inputs, then one encode_blocks(seal, link) call.
     Split: building the inputs, the call, and -- the same inputs resident in HBM -- the wall time of
     mv_dev_encode_blocks without seal (check, sizes, the total's read-back, the bytes) and with it.
     That wall time stands in for the device time of k_en_*: it bounds it from above.
  c  mv_dev_encode_blocks without seal over about 2^17 config-4-shape blocks resident in HBM, as GB/s
     of output, beside a device-to-device copy of the same number of bytes.

Each leg: `--warmup` runs, then the median of `--steps`; the whole measurement `--runs` times. Before
anything is printed b's blocks are held byte for byte against a's and against mv_verify_blocks, and
c's image against the host call's. Writes profiles/encode/encode_probe.json and prints it as one
JSON line.

    python tools/encode_probe.py [--rounds R] [--blocks N] [--steps K] [--warmup W] [--runs 2]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode", "encode_probe.json"))
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    eng = M.Engine(devices=(0,))
    n_auth, shape = 100, (67, 66, True)
    seeds = [MB.authority_seed(x) for x in range(n_auth)]
    seed_arr = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_auth, 32).copy()
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)

    # correctness first
    sealed = MB.build_rounds_sealed(eng, a.rounds, n_auth, seeds, *shape)
    encoded = MB.build_rounds_encoded(eng, a.rounds, n_auth, seeds, *shape)
    assert encoded == sealed, "build_rounds_encoded is not build_rounds_sealed"
    assert not eng.verify_blocks(encoded)[0].any(), "an encoded block does not verify"

    dev = torch.device("cuda", 0)

    def resident(rounds):
        heads, includes, (pbuf, poff, plen) = MB.encoded_inputs(rounds, n_auth, *shape)
        host = eng.encode_blocks(heads, includes, (pbuf, poff, plen))
        assert not host.status.any()
        n, cap = heads.shape[0], host.out_bytes
        t = {"n": n, "cap": cap, "host": host, "pbytes": pbuf.shape[0]}
        t["heads"] = torch.from_numpy(heads.view(np.int64)).to(dev)
        t["inc"] = torch.from_numpy(includes.view(np.int64)).to(dev)
        t["pay"] = torch.zeros(pbuf.shape[0] + 16, dtype=torch.uint8, device=dev)
        t["pay"][:pbuf.shape[0]] = torch.from_numpy(pbuf).to(dev)
        t["poff"], t["plen"] = torch.from_numpy(poff.view(np.int64)).to(dev), torch.from_numpy(plen.view(np.int64)).to(dev)
        t["out"] = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
        t["off"], t["len"] = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        t["st"], t["sst"] = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        return t

    def dev_encode(t, seal):
        total = eng.dev_encode_blocks(0, t["heads"], t["inc"], t["pay"], t["pbytes"], t["poff"], t["plen"], t["out"],
                                      t["cap"], t["off"], t["len"], t["st"], seal=seal, link=seal, d_seeds=d_seeds,
                                      d_seal_status=t["sst"])
        torch.cuda.synchronize()
        return total

    d_seeds = torch.from_numpy(seed_arr).to(dev)
    dag = resident(a.rounds)
    big = resident(max(1, a.blocks // n_auth))
    torch.cuda.synchronize()
    for t in (dag, big):
        assert dev_encode(t, False) == t["cap"]
        assert np.array_equal(t["out"][:t["cap"]].cpu().numpy(), t["host"].buf[:t["cap"]]), "device image != host image"
        assert not t["st"].any().item()
    assert dev_encode(dag, True) == dag["cap"] and not dag["sst"].any().item()
    assert dag["out"][:dag["cap"]].cpu().numpy().tobytes() == b"".join(
        b + bytes(-len(b) % 8) for b in sealed), "the sealed device image is not build_rounds_sealed's"
    copy_dst = torch.empty_like(big["out"])

    def dtod():
        copy_dst.copy_(big["out"])
        torch.cuda.synchronize()

    call_s = []
    inner = eng.encode_blocks

    def timed_call(*args, **kw):
        t0 = time.perf_counter()
        r = inner(*args, **kw)
        call_s.append(time.perf_counter() - t0)
        return r

    runs = []
    for _ in range(a.runs):
        ta = median_of(lambda: MB.build_rounds_sealed(eng, a.rounds, n_auth, seeds, *shape), a.warmup, a.steps)
        eng.encode_blocks = timed_call
        call_s.clear()
        tb = median_of(lambda: MB.build_rounds_encoded(eng, a.rounds, n_auth, seeds, *shape), a.warmup, a.steps)
        del eng.encode_blocks
        tcall = statistics.median(call_s[a.warmup:])
        tin = median_of(lambda: MB.encoded_inputs(a.rounds, n_auth, *shape), a.warmup, a.steps)
        tdev = median_of(lambda: dev_encode(dag, False), a.warmup, a.steps)
        tdev_seal = median_of(lambda: dev_encode(dag, True), a.warmup, a.steps)
        tc = median_of(lambda: dev_encode(big, False), a.warmup, a.steps)
        tcopy = median_of(dtod, a.warmup, a.steps)
        runs.append({
            "a_sealed_s_per_dag": ta, "b_encoded_s_per_dag": tb, "b_over_a_speedup": ta / tb,
            "b_inputs_s": tin, "b_call_s": tcall, "b_rest_s": tb - tin - tcall,
            "b_dev_encode_only_s": tdev, "b_dev_encode_seal_link_s": tdev_seal,
            "c_encode_s": tc, "c_encode_gb_per_s": big["cap"] / tc / 1e9, "c_dtod_gb_per_s": big["cap"] / tcopy / 1e9,
        })
    out = {"probe": "encode", "rounds": a.rounds, "dag_blocks": dag["n"], "dag_bytes": dag["cap"], "c_blocks": big["n"],
           "c_bytes": big["cap"], "steps": a.steps, "warmup": a.warmup, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
