"""Times of dot diffusion on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/dotdiff_bench.py [--repeats 10] [--quick]

  * dp_dotdiff_u8 per frame on 24 resident frames, 1080p and 4K, 16 and 256 colours, the default class matrix ("knuth"),
    strength 256, on image-like content (smooth ramps with grain), with the search table built ahead;
  * beside each, in the same process on the same batch and palette: Floyd-Steinberg (dp_error_diffusion_u8, no
    serpentine) -- what diffusion costs today -- and the nearest-only kernel (accelerator built) -- the floor of any mode
    that searches once per pixel.  Both per frame of the batch of 24 (throughput: the scan pipelines frames of a batch)
    and with ONE frame per call (latency: a scan has nothing to overlap with).
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
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

    classes, s256 = dl.DotDiffusionDitherStrategy()._settings()
    fs = dl.ErrorDiffusionDitherStrategy("floyd_steinberg", "false")
    cases = [("1080p", 1080, 1920, 16), ("1080p", 1080, 1920, 256), ("4K", 2160, 3840, 16), ("4K", 2160, 3840, 256)]
    if args.quick:
        cases = [("tiny", 147, 197, 16), ("tiny", 147, 197, 256)]
    for name, h, w, k in cases:
        frames = image_like(torch, N_FRAMES, h, w)
        out = torch.empty_like(frames)
        rs = np.random.RandomState(5 + k)
        P = be.Palette(*dl.prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], False))
        P.pattern_prepare()
        dot = profiled(be, torch, lambda: be.dotdiff(frames, P, classes, s256, out=out), 2 * R)
        ed = profiled(be, torch, lambda: fs._run(frames, P, out=out), max(2, R // 2), warmup=1)
        P.build_accel()
        near = profiled(be, torch, lambda: be.ordered(frames, P, be.MODE_NEAREST, out=out), R)
        ed_ms, near_ms = float(np.median(ed)) / N_FRAMES, float(np.median(near)) / N_FRAMES
        # one frame per call: what an image, or a stream that dithers frame by frame, waits for (the product's tile edge)
        one_in, one_out = frames[:1].clone(), torch.empty_like(frames[:1])
        one = {"dotdiff_ms": stats(profiled(be, torch, lambda: be.dotdiff(one_in, P, classes, s256, out=one_out), R))["median_ms"],
               "floyd_steinberg_ms": stats(profiled(be, torch, lambda: fs._run(one_in, P, out=one_out), max(2, R // 2), warmup=1))["median_ms"],
               "nearest_only_ms": stats(profiled(be, torch, lambda: be.ordered(one_in, P, be.MODE_NEAREST, out=one_out), R))["median_ms"]}
        one["ratio_to_floyd_steinberg"] = round(one["dotdiff_ms"] / one["floyd_steinberg_ms"], 4)
        rec = {"what": f"dp_dotdiff_u8 {name} {k} colours, knuth matrix, 24 frames, image-like, strength 256",
               "floyd_steinberg_ms_per_frame": round(ed_ms, 4), "nearest_only_ms_per_frame": round(near_ms, 4), "one_frame_per_call": one}
        s = stats(dot)
        per, t = s["median_ms"] / N_FRAMES, be.DOTDIFF_TILE
        rec["batch"] = {"ms_per_frame": round(per, 4), "p10": round(s["p10_ms"] / N_FRAMES, 4), "p90": round(s["p90_ms"] / N_FRAMES, 4),
                        "repeats": s["repeats"], "tile": t, "redone_pixels": round((t + 32) ** 2 / t ** 2, 2),
                        "ratio_to_floyd_steinberg": round(per / ed_ms, 4), "ratio_to_nearest_only": round(per / near_ms, 2)}
        print(json.dumps(rec), flush=True)
        del frames, out, P
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
