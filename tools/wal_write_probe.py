"""What the device WAL write costs: mv_dev_wal_write on HBM-resident blocks, its layout alone, the
replay's crc pass over the image it wrote, and the host's way to the same bytes.

Input: N config-4-shape blocks (as bench_blocks.py builds them: 100 authorities, 67 includes, one
512-B Share, 66 VoteRanges; 4,100 distinct blocks tiled to N, every copy at its own place in HBM)
written as WAL entries at 16-MiB maps, every 128th an own block (tag 3), the rest tag 1. Each of
these is warmed up and then timed `--steps` times (the median is reported):

  write    mv_dev_wal_write and a device synchronise behind it: layout, gaps, headers, bodies, crc
  layout   the same call with cap = 0: the checks, the scan, the crossings and the positions
  emit     write - layout (the byte pass; a difference of medians, not a measurement of its own)
  crc      k_wal_crc's stage time in one mv_dev_wal_verify of the image (run once: mv_stage_times)
  host     zlib.crc32 of every body and the copy of header and body into a host image, on 16
           threads, over the first --host-blocks entries (run once)

The image is checked: mv_dev_wal_verify finds N entries, all MV_WAL_OK, at the written positions,
and the first and the last entries equal the image the host leg writes (each check is reported). Prints one JSON line.

    python tools/wal_write_probe.py [--blocks N] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-bits", type=int, default=24)
    ap.add_argument("--host-blocks", type=int, default=1 << 16)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import mysticeti_amd as M
    import mysticeti_amd.blocks as MB

    eng = M.Engine(devices=(0,))
    dev = torch.device("cuda:0")
    base = MB.config4(eng, rounds=41)  # 4,100 distinct blocks
    n, bits = a.blocks, a.map_bits
    base_buf, base_off, base_len = MB.pack(base)
    base_bytes = int(base_off[-1] + base_len[-1])
    reps = (n + len(base) - 1) // len(base)
    d_base = torch.from_numpy(base_buf[:base_bytes].copy()).to(dev)
    d_buf = torch.zeros(reps * base_bytes + 16, dtype=torch.uint8, device=dev)
    d_buf[:reps * base_bytes] = d_base.repeat(reps)
    idx = np.arange(n)
    rows = np.zeros((n, 4), dtype=np.uint64)
    own = idx % 128 == 5
    rows[:, 0] = np.where(own, 3, 1)
    rows[:, 1] = base_off[idx % len(base)] + (idx // len(base)).astype(np.uint64) * np.uint64(base_bytes)
    rows[:, 2] = base_len[idx % len(base)]
    rows[:, 3] = idx
    body = rows[:, 2] + np.where(own, 8, 0).astype(np.uint64)
    pos, end = M.wal_layout(body, bits)
    d_rows = torch.from_numpy(rows.view(np.int64).copy()).to(dev)
    d_out = torch.zeros(end + 16, dtype=torch.uint8, device=dev)
    d_pos = torch.zeros(n, dtype=torch.int64, device=dev)
    buf_bytes = reps * base_bytes

    def write():
        assert eng.dev_wal_write(0, d_buf, buf_bytes, d_rows, 0, bits, d_out, end, d_pos) == end
        torch.cuda.synchronize()

    def layout():
        assert eng.dev_wal_write(0, d_buf, buf_bytes, d_rows, 0, bits, None, 0, d_pos) == end

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    t_write, t_layout = timed(write), timed(layout)
    # the checked call, and the replay's crc pass over its image
    d_out.zero_()
    d_pos.zero_()
    write()
    cap = n + 8
    d_epos = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_tag, d_len = torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev)
    d_st = torch.full((cap,), 255, dtype=torch.uint8, device=dev)
    eng.dev_wal_verify(0, d_out, end, end, bits, d_epos, d_tag, d_len, d_st, cap)  # warm-up
    eng.set_stage_timing(True)
    eng.stage_times(reset=True)
    cnt = eng.dev_wal_verify(0, d_out, end, end, bits, d_epos, d_tag, d_len, d_st, cap)
    stage_ms = {k: round(v, 3) for k, v in eng.stage_times(reset=True)[0].items() if v}
    eng.set_stage_timing(False)
    got_pos = d_pos.cpu().numpy().view(np.uint64)
    k = min(int(cnt), n)
    checks = {"pos_equal_wal_layout": bool(np.array_equal(got_pos, pos)), "verify_count": bool(cnt == n),
              "verify_pos": bool(np.array_equal(d_epos[:k].cpu().numpy().view(np.uint64), pos[:k])),
              "verify_all_ok": not bool(d_st[:k].any()),
              "verify_len": bool(np.array_equal(d_len[:k].cpu().numpy().astype(np.uint64), body[:k]))}

    # the host's way: crc and copy, 16 threads over contiguous runs of entries
    hn = min(n, a.host_blocks)
    h_end = int(pos[hn - 1] + 16 + body[hn - 1])
    h_img = np.zeros(h_end, dtype=np.uint8)

    def run(lo, hi, img=None, origin=0):
        img = h_img if img is None else img
        for i in range(lo, hi):
            b = base[i % len(base)]
            payload = (struct.pack("<Q", i) + b) if own[i] else b
            p = int(pos[i]) - origin
            img[p:p + 16] = np.frombuffer(struct.pack("<QII", zlib.crc32(payload), len(payload) + 16, 3 if own[i] else 1),
                                          dtype=np.uint8)
            img[p + 16:p + 16 + len(payload)] = np.frombuffer(payload, dtype=np.uint8)

    cuts = [hn * k // 16 for k in range(17)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda k: run(cuts[k], cuts[k + 1]), range(16)))
    host_ms = (time.perf_counter() - t0) * 1e3
    checks["first_entries_equal_host_image"] = bool(np.array_equal(d_out[:h_end].cpu().numpy(), h_img))
    # the image's last entries (past 4 GiB at the default size), against the same host writer
    t0 = max(n - 4096, 0)
    origin = int(pos[t0])
    t_img = np.zeros(end - origin, dtype=np.uint8)
    run(t0, n, t_img, origin)
    checks["last_entries_equal_host_image"] = bool(np.array_equal(d_out[origin:end].cpu().numpy(), t_img))
    ok = all(checks.values())

    med = lambda v: round(float(np.median(v)), 3)
    w, l = med(t_write), med(t_layout)
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 2) if ms > 0 else None
    print(json.dumps({"probe": "wal_write", "blocks": n, "map_bits": bits, "image_bytes": int(end),
                      "maps_crossed": int(end >> bits),
                      "write_ms": {"median": w, "min": round(min(t_write), 3), "max": round(max(t_write), 3)},
                      "layout_ms": {"median": l, "min": round(min(t_layout), 3), "max": round(max(t_layout), 3)},
                      "emit_ms_by_difference": round(w - l, 3),
                      "write_image_GB_per_s": gbs(end, w), "emit_image_GB_per_s": gbs(end, w - l),
                      "verify_stages_ms_once": stage_ms, "wal_crc_image_GB_per_s": gbs(end, stage_ms.get("wal_crc", 0)),
                      "host16_blocks": hn, "host16_ms_once": round(host_ms, 3), "host16_image_GB_per_s": gbs(h_end, host_ms),
                      "results_equal_and_ok": ok, "checks": checks, "steps": a.steps, "warmup": a.warmup}))
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
