"""Times of the Oklab palette fit on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/okfit_bench.py [--repeats 10] [--quick] [--out FILE]

For the colour histogram of ONE image-like frame (smooth ramps with grain) at 1080p and at 4K, and 16 and 256 colours:
  * count and compact: dp_okfit_hist_points into a buffer of exactly n records (two scans of the table and a prefix);
  * the seeding: the "main" part of dp_okfit_fit's events (K launches and the last pick);
  * a Lloyd pass: the difference of the "fix-up" parts (passes + medoids) of a fit cut at 11 passes and of one cut at 1 pass,
    over 10 -- a pass as the fit runs it: the assignment launch, the update launch and the host's read of one word;
  * the whole fit (max_iter 100): both parts, with the number of passes it took;
  * beside them, by the host's clock around the synchronous calls, in the same process on the same histogram:
    ClipPalette.oklab and ClipPalette.kmeans (the float64 k-means over the histogram, sklearn's stopping rule).
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def image_like(torch, h, w):
    """Smooth ramps with grain, generated on the device (as tools/bench_scripts/idiff_bench.py)."""
    y = torch.arange(h, device="cuda").view(h, 1).float()
    x = torch.arange(w, device="cuda").view(1, w).float()
    g = torch.Generator(device="cuda").manual_seed(1)
    ch = [(x * (200.0 / w) + 20), (y * (180.0 / h) + 30), ((x + y) * (150.0 / (w + h)) + 40)]
    f = torch.stack([c.expand(h, w) for c in ch], dim=-1)
    f = f + torch.randint(0, 3, f.shape, device="cuda", generator=g).float()
    return f.clamp_(0, 255).to(torch.uint8).contiguous()


def profiled(be, torch, fn, repeats, warmup=2):
    """-> per-call (main, fix-up) ms of the library's own events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    be.profile_enable(True)
    be.profile_read()
    out = []
    for _ in range(repeats):
        fn()
        a, b, _ = be.profile_read()
        out.append((a, b))
    be.profile_enable(False)
    return np.array(out)


def wall(torch, fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="a small frame, two repeats: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import _lib
    from dither_pie_amd import backend as be
    from dither_pie_amd.clip_palette import ClipPalette
    assert torch.cuda.is_available(), "needs a HIP device"
    R = 2 if args.quick else args.repeats
    L = _lib.load()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    warm = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    for _ in range(20 if args.quick else 200):   # warm clocks
        warm[: 128 << 20].copy_(warm[128 << 20:])
    torch.cuda.synchronize()
    del warm

    sizes = [("1080p", 1080, 1920), ("4K", 2160, 3840)]
    if args.quick:
        sizes = [("tiny", 147, 197)]
    for name, h, w in sizes:
        clip = ClipPalette().add(image_like(torch, h, w))
        hist = clip._hist
        n = hist.n_occupied()
        pts = torch.empty((n, be.OKFIT_POINT_BYTES), dtype=torch.uint8, device="cuda")
        n_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(L.dp_okfit_hist_workspace_bytes(), dtype=torch.uint8, device="cuda")

        def compact():
            be.check(L.dp_okfit_hist_points(hist.buf.data_ptr(), pts.data_ptr(), n, n_dev.data_ptr(), ws.data_ptr(), ws.numel(), be._stream()))

        emit({"what": f"count and compact, {name} image-like frame", "pixels": h * w, "distinct_colours": n,
              **stats(profiled(be, torch, compact, R).sum(1))})
        for K in (16, 256):
            cut1 = profiled(be, torch, lambda: be.okfit(pts, K, 1), R)
            cut11 = profiled(be, torch, lambda: be.okfit(pts, K, 11), R)
            full = profiled(be, torch, lambda: be.okfit(pts, K, 100), max(2, R // 2), warmup=1)
            n_iter, n_iter11 = be.okfit(pts, K, 100)[2], be.okfit(pts, K, 11)[2]
            per_pass = (np.median(cut11[:, 1]) - np.median(cut1[:, 1])) / max(n_iter11 - 1, 1)
            emit({"what": f"dp_okfit_fit, {name} image-like frame, {K} colours", "distinct_colours": n,
                  "seeding": stats(np.concatenate([cut1[:, 0], cut11[:, 0]])), "lloyd_pass_ms": round(float(per_pass), 4), "passes_in_the_cut_fit": n_iter11,
                  "whole_fit": stats(full.sum(1)), "whole_fit_passes": n_iter})
            ok_wall = stats(wall(torch, lambda: clip.oklab(K), max(2, R // 2)))
            km_wall = stats(wall(torch, lambda: clip.kmeans(K), max(2, R // 2)))
            km_iter = clip.kmeans_fit(K)[3]
            emit({"what": f"host clock, {name} image-like frame, {K} colours", "ClipPalette.oklab": ok_wall, "oklab_passes": n_iter,
                  "ClipPalette.kmeans": km_wall, "kmeans_iterations": int(km_iter)})
        del clip, hist, pts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
