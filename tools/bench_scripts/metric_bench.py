"""Times of the Oklab colour metric on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/metric_bench.py [--repeats 10] [--quick]

  * the build of the 2^24-entry top-2 table (dp_metric_prepare, synchronous: host clock around it, and the build kernel inside
    it from the library's events) for a 16- and a 256-colour palette, with the cube root as a float estimate corrected in
    integers (the product) and as a gather from a 65536-entry table (DP_METRIC_CBRT_TABLE, experiments build);
  * dp_metric_ordered_u8 per frame on 24 resident frames, 1080p and 4K, 16 and 256 colours, image-like content (smooth ramps
    with grain), DP_MODE_NEAREST and DP_MODE_MATRIX (Bayer 8 x 8), with both cube roots (alternating, same session);
  * beside each: dp_ordered_u8 with an RGB palette of the same size (accelerator built) on the same batch, same process;
  * pattern dithering at m = 4 on both palettes.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys
import time

os.environ["DITHER_PIE_EXPERIMENTS"] = "1"          # the twin library: the only build that reads DP_METRIC_CBRT_TABLE

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24


def stats(ms, per=1):
    a = np.sort(np.asarray(ms, np.float64)) / per
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device (as tools/bench_scripts/pattern_bench.py)."""
    y = torch.arange(h, device="cuda").view(1, h, 1).float()
    x = torch.arange(w, device="cuda").view(1, 1, w).float()
    t = torch.arange(n, device="cuda").view(n, 1, 1).float()
    g = torch.Generator(device="cuda").manual_seed(1)
    ch = [(x * (200.0 / w) + t * 2 + 20), (y * (180.0 / h) + t + 30), ((x + y) * (150.0 / (w + h)) + 40)]
    f = torch.stack([c.expand(n, h, w) for c in ch], dim=-1)
    f = f + torch.randint(0, 3, f.shape, device="cuda", generator=g).float()
    return f.clamp_(0, 255).to(torch.uint8).contiguous()


def profiled(be, torch, fn, repeats, warmup=2):
    """-> per-call (main + fix-up) ms of the library's own events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    be.profile_enable(True)
    be.profile_read()
    out = []
    for _ in range(repeats):
        fn()
        a, b, _ = be.profile_read()
        out.append(a + b)
    be.profile_enable(False)
    return out


def palette_values(k):
    return np.random.RandomState(5 + k).randint(0, 256, (k, 3)).astype(np.float32)


def metric_palette(be, k, cbrt_table):
    """A metric palette whose table (built at the first use) and kernels take the cube root from a table or from the estimate."""
    if cbrt_table:
        os.environ["DP_METRIC_CBRT_TABLE"] = "1"
    else:
        os.environ.pop("DP_METRIC_CBRT_TABLE", None)
    pal = palette_values(k)
    P = be.Palette(pal, pal.astype(np.uint8), metric="oklab")
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small frames, two repeats: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import backend as be
    from dither_pie_amd import dithering_lib as dl
    assert torch.cuda.is_available(), "needs a HIP device"
    R = 2 if args.quick else args.repeats

    warm = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    for _ in range(20 if args.quick else 200):   # warm clocks
        warm[: 128 << 20].copy_(warm[128 << 20:])
    torch.cuda.synchronize()
    del warm

    # ---- the table build
    for k in (16, 256):
        for cbrt_table in (False, True):
            wall, kern = [], []
            for i in range(3):
                P = metric_palette(be, k, cbrt_table)
                torch.cuda.synchronize()
                be.profile_enable(True)
                be.profile_read()
                t = time.perf_counter()
                P.metric_prepare()
                wall.append((time.perf_counter() - t) * 1e3)
                a, b, _ = be.profile_read()
                be.profile_enable(False)
                kern.append(a + b)
                del P
            print(json.dumps({"what": f"dp_metric_prepare, {k} colours, cube root by {'table' if cbrt_table else 'estimate'}",
                              "wall_ms_runs": [round(v, 3) for v in wall], "build_kernel_ms_runs": [round(v, 3) for v in kern]}), flush=True)
    os.environ.pop("DP_METRIC_CBRT_TABLE", None)

    # ---- the per-pixel kernel, both cube roots, and the RGB ordered kernel; pattern m = 4 on both palettes
    bayer8 = be.Thresholds.from_matrix(dl.DitherUtils.get_threshold_matrix(dl.DitherMode.BAYER, "8x8"))
    cases = [("1080p", 1080, 1920), ("4K", 2160, 3840)]
    if args.quick:
        cases = [("tiny", 67, 129)]
    for name, h, w in cases:
        frames = image_like(torch, N_FRAMES, h, w)
        out = torch.empty_like(frames)
        for k in (16, 256):
            pals = {"estimate": metric_palette(be, k, False)}
            pals["estimate"].metric_prepare()
            pals["table"] = metric_palette(be, k, True)
            pals["table"].metric_prepare()
            os.environ.pop("DP_METRIC_CBRT_TABLE", None)
            pv = palette_values(k)
            rgb = be.Palette(pv, pv.astype(np.uint8))
            rgb.build_accel()
            rec = {"what": f"ordered {name} {k} colours, 24 frames, image-like; ms per frame"}
            for mode_name, mode, thr in (("nearest", be.MODE_NEAREST, None), ("matrix_bayer8", be.MODE_MATRIX, bayer8)):
                res = {"estimate": [], "table": []}
                for which in ("estimate", "table", "estimate", "table"):   # alternating
                    res[which] += profiled(be, torch, lambda: be.ordered(frames, pals[which], mode, thr=thr, out=out), R)
                assert torch.equal(be.ordered(frames, pals["estimate"], mode, thr=thr), be.ordered(frames, pals["table"], mode, thr=thr))
                for which in res:
                    rec[f"metric_{mode_name}_cbrt_{which}"] = stats(res[which], N_FRAMES)
                rec[f"rgb_{mode_name}"] = stats(profiled(be, torch, lambda: be.ordered(frames, rgb, mode, thr=thr, out=out), R), N_FRAMES)
            pals["estimate"].pattern_prepare()
            rgb.pattern_prepare()
            rec["pattern_m4_metric"] = stats(profiled(be, torch, lambda: be.pattern(frames, pals["estimate"], 4, 128, out=out), R), N_FRAMES)
            rec["pattern_m4_rgb"] = stats(profiled(be, torch, lambda: be.pattern(frames, rgb, 4, 128, out=out), R), N_FRAMES)
            print(json.dumps(rec), flush=True)
            del pals, rgb
        del frames, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
