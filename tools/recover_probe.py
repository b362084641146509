"""What seeding the DAG store from a replayed WAL costs, on tools/replay_probe.py's image in HBM.

Input: N config-4-shape blocks (100 authorities, 67 includes, one 512-B Share, 66 VoteRanges; 4,100
distinct blocks, repeated) as WAL entries at 16-MiB maps, every 128th an own block. Three paths over
the same bytes on a cleared context with the genesis references seeded, each warmed up and then
timed `--steps` times (the median is reported; mv_index_clear and the genesis seeding are outside
the timed region):

  a  mv_dev_wal_replay + mv_dev_index_insert(rows + 3, 10, MV_REF_STORED): the record-less seeding
  b  mv_dev_wal_replay + mv_dev_dag_seed_rows: references, records and edges
  c  mv_dev_wal_replay for the rows, then the same blocks through mv_dev_connect_blocks with the DAG
     store on -- the only other way to those records, which verifies every block a second time; the
     replay is outside its timed region

b - a is what the records cost; c is what they cost without the seed call. Prints one JSON line.

    python tools/recover_probe.py [--blocks N] [--steps K] [--warmup W]
"""
import argparse
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
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    eng = M.Engine(devices=(0,))
    base = MB.config4(eng, rounds=41)  # 4,100 distinct blocks
    n_auth = 100
    pks, stakes = MB.committee(eng, n_auth, distinct=True)
    eng.set_committee(pks, stakes, 0)
    genesis = MB.genesis_refs(n_auth)
    n, bits = a.blocks, a.map_bits
    own = lambda i: i % 128 == 5
    plen = np.array([len(base[i % len(base)]) + (8 if own(i) else 0) for i in range(n)], dtype=np.uint64)
    pos, end = M.wal_layout(plen, bits)
    image = np.zeros(end + 64, dtype=np.uint8)
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
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(image).to(dev)
    cap = n + 8
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    out = dict(d_pos=i64(cap), d_tag=torch.zeros(cap, dtype=torch.int32, device=dev),
               d_len=torch.zeros(cap, dtype=torch.int32, device=dev), d_status=u8(cap), d_rows=i64(cap, 10),
               d_blk_status=u8(cap), d_summary=i64(3), d_last_seen=i64(n_auth))
    d_st, d_state, d_missing, d_connected = u8(cap), u8(cap), i64(8, 6), i64(cap, 8)
    distinct = min(n, len(base))
    incs = sum(len(b) >= 64 and struct.unpack_from("<Q", b, 56)[0] for b in base[:distinct])
    all_incs = sum(struct.unpack_from("<Q", base[i % len(base)], 56)[0] for i in range(n))
    eng.index_reserve(2 * (n + all_incs) + 1024)
    eng.pending_reserve(n, all_incs)
    eng.dag_reserve(n, all_incs)

    def fresh():
        eng.index_clear()
        eng.index_insert_stored(genesis)

    def replay():
        cnt, nb = eng.dev_wal_replay(0, d_img, end, end, bits, **out)
        assert (cnt, nb) == (n, n), (cnt, nb)

    def path_a():
        replay()
        eng.dev_index_insert(0, out["d_rows"], 10, n, M.REF_STORED, word_offset=3)
        torch.cuda.synchronize(dev)

    seeded = {}

    def path_b():
        replay()
        seeded["b"] = eng.dev_dag_seed_rows(0, d_img, end, out["d_rows"], out["d_blk_status"], n_rows=n).words()

    def path_c():
        seeded["c"] = eng.dev_connect_blocks(0, d_img, end, d_off, d_len, None, d_st[:n], d_state[:n], d_missing, d_connected)

    def timed(fn, before=fresh):
        ms = []
        for k in range(a.warmup + a.steps):
            before()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    t_a = timed(path_a)
    stats_a = (eng.pending_stats().stored, eng.dag_stats().records)
    t_b = timed(path_b)
    stats_b = (eng.pending_stats().stored, eng.dag_stats().records, eng.dag_stats().includes)
    replay()
    d_off, d_len = out["d_rows"][:n, 1].contiguous(), out["d_rows"][:n, 2].contiguous()
    t_c = timed(path_c)
    stats_c = (eng.pending_stats().stored, eng.dag_stats().records, eng.dag_stats().includes)
    ok = (stats_a == (distinct + n_auth, 0) and stats_b == (distinct + n_auth, distinct, incs) and stats_c == stats_b
          and seeded["b"] == [n, distinct, incs, 0, 0] and seeded["c"] == (0, distinct))
    med = lambda v: round(float(np.median(v)), 3)
    span = lambda v: {"median": med(v), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps({"probe": "recover", "blocks": n, "distinct_blocks": distinct, "records": stats_b[1], "includes": stats_b[2],
                      "map_bits": bits, "image_bytes": int(end), "a_replay_index_insert_ms": span(t_a),
                      "b_replay_seed_rows_ms": span(t_b), "c_connect_blocks_ms": span(t_c),
                      "b_minus_a_ms": round(med(t_b) - med(t_a), 3),
                      "c_over_b_minus_a": round(med(t_c) / max(med(t_b) - med(t_a), 1e-3), 2),
                      "results_equal_and_ok": ok, "steps": a.steps, "warmup": a.warmup}))
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
