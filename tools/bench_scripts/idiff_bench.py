"""Times of integer error diffusion on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/idiff_bench.py [--repeats 10] [--quick] [--out FILE]

  * dp_idiff_u8 at 1080p and 4K, 16 and 256 colours, under the RGB metric and under Oklab, Floyd-Steinberg and JJN,
    strength 256, on image-like content (smooth ramps with grain), with the search tables built ahead: ONE frame per call
    (latency: a scan has nothing to overlap with) and per frame of 24 resident frames (throughput: one workgroup per frame);
  * beside each RGB figure, in the same process on the same frames and palette: dp_error_diffusion_u8 with the same variant
    (no serpentine) -- the float scan this mode stands next to -- and dp_dotdiff_u8 (the default class matrix);
  * one A/B, in the experiments library: 16-step against 8-step I/O periods (DP_IDIFF_PERIOD), alternating in one process.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24


def stats(ms, per=1):
    a = np.sort(np.asarray(ms, np.float64)) / per
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device (as tools/bench_scripts/dotdiff_bench.py)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small frames, two repeats: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import _lib
    from dither_pie_amd import backend as be
    from dither_pie_amd import dithering_lib as dl
    assert torch.cuda.is_available(), "needs a HIP device"
    R = 2 if args.quick else args.repeats

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

    classes, dot256 = dl.DotDiffusionDitherStrategy()._settings()
    sizes = [("1080p", 1080, 1920), ("4K", 2160, 3840)]
    if args.quick:
        sizes = [("tiny", 147, 197)]
    for name, h, w in sizes:
        frames = image_like(torch, N_FRAMES, h, w)
        out = torch.empty_like(frames)
        one_in, one_out = frames[:1].clone(), torch.empty_like(frames[:1])
        for k in (16, 256):
            rs = np.random.RandomState(5 + k)
            spec = dl.prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], False)
            pals = {"rgb": be.Palette(*spec), "oklab": be.Palette(spec[0], spec[1], metric="oklab")}
            pals["oklab"].metric_prepare()
            for P in pals.values():
                P.pattern_prepare()
            dot_one = stats(profiled(be, torch, lambda: be.dotdiff(one_in, pals["rgb"], classes, dot256, out=one_out), R))
            dot_batch = stats(profiled(be, torch, lambda: be.dotdiff(frames, pals["rgb"], classes, dot256, out=out), R), N_FRAMES)
            for variant in ("floyd_steinberg", "jjn"):
                taps, divisor, s256 = dl.IntegerErrorDiffusionDitherStrategy(variant)._settings()
                fl = dl.ErrorDiffusionDitherStrategy(variant, "false")
                P = pals["rgb"]
                float_one = stats(profiled(be, torch, lambda: fl._run(one_in, P, out=one_out), max(2, R // 2), warmup=1))
                float_batch = stats(profiled(be, torch, lambda: fl._run(frames, P, out=out), max(2, R // 2), warmup=1), N_FRAMES)
                for metric, P in pals.items():
                    one = stats(profiled(be, torch, lambda: be.idiff(one_in, P, taps, divisor, s256, out=one_out), R))
                    batch = stats(profiled(be, torch, lambda: be.idiff(frames, P, taps, divisor, s256, out=out), R), N_FRAMES)
                    rec = {"what": f"dp_idiff_u8 {name} {k} colours {metric} {variant}, image-like, strength 256",
                           "one_frame_per_call": one, "per_frame_of_24": batch,
                           "float_scan_one_frame_ms": float_one["median_ms"], "float_scan_per_frame_of_24_ms": float_batch["median_ms"],
                           "ratio_to_float_scan_one_frame": round(one["median_ms"] / float_one["median_ms"], 4),
                           "ratio_to_float_scan_per_frame_of_24": round(batch["median_ms"] / float_batch["median_ms"], 4),
                           "dotdiff_one_frame_ms": dot_one["median_ms"], "dotdiff_per_frame_of_24_ms": dot_batch["median_ms"]}
                    emit(rec)
            del pals
        # the A/B: I/O periods of 16 and of 8 steps, the experiments library, alternating
        dl.drop_device_caches()
        prev = _lib.select(True)
        try:
            rs = np.random.RandomState(5 + 16)
            P = be.Palette(*dl.prepare_palette([tuple(c) for c in rs.randint(0, 256, (16, 3)).tolist()], False))
            P.pattern_prepare()
            for variant in ("floyd_steinberg", "jjn"):
                taps, divisor, s256 = dl.IntegerErrorDiffusionDitherStrategy(variant)._settings()
                got = {"16": {"one": [], "batch": []}, "8": {"one": [], "batch": []}}
                for _ in range(3):
                    for period in ("16", "8"):
                        os.environ["DP_IDIFF_PERIOD"] = period
                        got[period]["one"] += profiled(be, torch, lambda: be.idiff(one_in, P, taps, divisor, s256, out=one_out), max(2, R // 2), warmup=1)
                        got[period]["batch"] += profiled(be, torch, lambda: be.idiff(frames, P, taps, divisor, s256, out=out), max(2, R // 2), warmup=1)
                emit({"what": f"A/B I/O period, dp_idiff_u8 {name} 16 colours rgb {variant} (experiments library)",
                      "period_16": {"one_frame_per_call": stats(got["16"]["one"]), "per_frame_of_24": stats(got["16"]["batch"], N_FRAMES)},
                      "period_8": {"one_frame_per_call": stats(got["8"]["one"]), "per_frame_of_24": stats(got["8"]["batch"], N_FRAMES)}})
            del P
        finally:
            os.environ.pop("DP_IDIFF_PERIOD", None)
            dl.drop_device_caches()
            _lib.select(prev)
        del frames, out, one_in, one_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
