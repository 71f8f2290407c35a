"""Times of the void-and-cluster generator on one MI355X (device events around each call; warm clocks; median [p10-p90]).

  python tools/bench_scripts/voidcluster_bench.py [--repeats 10] [--quick]

  * dp_void_cluster_u16 at 64 x 64 and 128 x 128, sigma 1.5, with 1 and with 64 matrices per call (one workgroup each:
    64 matrices occupy 64 of the 256 compute units);
  * beside them, in the same process: Thresholds.void_cluster (the same launch plus download, step 6 and the uploads) and
    Thresholds.blue_noise at the same size -- the comparison: as many rounds of argmin-and-update over as many cells, in one
    workgroup of 1024 lanes as well.  Per round: the call divided by h * w.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def timed(torch, fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small matrices, two repeats: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import backend as be
    assert torch.cuda.is_available(), "needs a HIP device"
    R = 2 if args.quick else args.repeats

    warm = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    for _ in range(20 if args.quick else 200):   # warm clocks
        warm[: 128 << 20].copy_(warm[128 << 20:])
    torch.cuda.synchronize()
    del warm

    for size in ((16, 32) if args.quick else (64, 128)):
        n = size * size
        rec = {"what": f"void-and-cluster {size} x {size}, sigma 1.5", "rounds": n}
        for count in (1, 64):
            out = torch.empty((count, size, size), dtype=torch.int16, device="cuda")
            seeds = list(range(100, 100 + count))
            s = stats(timed(torch, lambda: be.void_cluster_ranks(size, size, seeds, 1.5, out=out), R))
            s["us_per_round"] = round(1e3 * s["median_ms"] / n, 3)
            rec[f"dp_void_cluster_u16_{count}"] = s
        rec["thresholds_void_cluster"] = stats(timed(torch, lambda: be.Thresholds.void_cluster(size, size, 42, 1.5), R))
        bn = stats(timed(torch, lambda: be.Thresholds.blue_noise(size, 42), R))
        bn["us_per_round"] = round(1e3 * bn["median_ms"] / n, 3)
        rec["thresholds_blue_noise"] = bn
        rec["round_ratio_to_blue_noise"] = round(rec["dp_void_cluster_u16_1"]["median_ms"] / bn["median_ms"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
