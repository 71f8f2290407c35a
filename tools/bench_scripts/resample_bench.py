"""Times of the filtered resize on one MI355X (warm clocks; median [p10-p90]).

  python tools/bench_scripts/resample_bench.py [--repeats 10] [--quick] [--out FILE]

  * dp_resample_u8, box and lanczos, on resident image-like frames: 24 4K frames -> 1080p (597 MB of input: more than the
    Infinity Cache), 24 1080p frames -> the pixelization geometries of max_size 64 (64 x 114) and 270 (270 x 480).  Per frame:
    the horizontal and the vertical pass from the library's own HIP events (dp_profile_*), the whole call from events around it;
    input + intermediate + output bytes over the call's time as a fraction of the HBM peak (8 TB/s);
  * beside it, in the same process on the same frames: dp_resize_nearest_u8 (it reads a fraction of the bytes: a floor, not a
    target) and Image.resize of one frame on the host;
  * process_frames end to end (Bayer 4x4, 16 colours, no enlargement) with the filter and with NEAREST;
  * the A/B of the horizontal pass in the experiments library, alternating in one process: the staged kernel against the naive
    one (DP_RESAMPLE_H=staged / naive), whichever of the two the planner's rule gives the plan.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24
HBM_PEAK_BYTES_PER_S = 8.0e12


def stats(ms, per=1):
    a = np.sort(np.asarray(ms, np.float64)) / per
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device frame by frame (as tools/bench_scripts/idiff_bench.py)."""
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    y = torch.arange(h, device="cuda").view(h, 1).float()
    x = torch.arange(w, device="cuda").view(1, w).float()
    g = torch.Generator(device="cuda").manual_seed(1)
    for t in range(n):
        ch = [(x * (200.0 / w) + t * 2 + 20), (y * (180.0 / h) + t + 30), ((x + y) * (150.0 / (w + h)) + 40)]
        f = torch.stack([c.expand(h, w) for c in ch], dim=-1)
        f = f + torch.randint(0, 3, f.shape, device="cuda", generator=g).float()
        out[t] = f.clamp_(0, 255).to(torch.uint8)
    return out


def timed(torch, fn, repeats, warmup=2):
    """-> per-call ms between two events around the call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def passes(be, torch, fn, repeats, warmup=2):
    """-> (horizontal ms, vertical ms) per call from the library's events (the launcher marks the boundary between the passes)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    be.profile_enable(True)
    be.profile_read()
    hs, vs = [], []
    for _ in range(repeats):
        fn()
        a, b, _ = be.profile_read()
        hs.append(a)
        vs.append(b)
    be.profile_enable(False)
    return hs, vs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small frames, two repeats: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from PIL import Image
    from dither_pie_amd import _lib
    from dither_pie_amd import backend as be
    from dither_pie_amd import dithering_lib as dl
    from dither_pie_amd import video_processor as vp
    assert torch.cuda.is_available(), "needs a HIP device"
    R = 2 if args.quick else args.repeats
    n = 3 if args.quick else N_FRAMES
    pil = {"box": Image.BOX, "lanczos": Image.LANCZOS}

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

    def geom(h, w, max_size):
        tw, th = vp._even_dimensions(w, h, max_size)
        return th, tw

    work = [("4K -> 1080p", 2160, 3840, 1080, 1920), ("1080p -> max_size 64", 1080, 1920) + geom(1080, 1920, 64),
            ("1080p -> max_size 270", 1080, 1920) + geom(1080, 1920, 270)]
    if args.quick:
        work = [("tiny", 147, 197, 40, 54)]
    dith = dl.ImageDitherer(16, dl.DitherMode.BAYER, [tuple(int(v) for v in c) for c in np.random.RandomState(3).randint(0, 256, (16, 3))], False,
                            {"size": "4x4"})
    staged = []
    frames, shape = None, None
    for label, h, w, oh, ow in work:
        if shape != (h, w):
            del frames
            torch.cuda.empty_cache()
            frames, shape = image_like(torch, n, h, w), (h, w)
        out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        near = stats(timed(torch, lambda: be.resize_nearest(frames, oh, ow), R), n)
        host_frame = frames[0].cpu().numpy()
        for name in ("box", "lanczos"):
            plan = be.ResamplePlan(name, h, w, oh, ow)
            mid = plan.workspace_bytes(n)
            whole = stats(timed(torch, lambda: be.resample(frames, oh, ow, name, out=out, plan=plan), R), n)
            hs, vs = passes(be, torch, lambda: be.resample(frames, oh, ow, name, out=out, plan=plan), R)
            moved = frames.numel() + 2 * mid + out.numel()      # the intermediate is written, then read
            t0 = time.perf_counter()
            for _ in range(max(1, R // 2)):
                Image.fromarray(host_frame, "RGB").resize((ow, oh), pil[name])
            host_ms = (time.perf_counter() - t0) * 1e3 / max(1, R // 2)
            emit({"what": f"dp_resample_u8 {label} ({h}x{w} -> {oh}x{ow}) {name}, {n} resident image-like frames", "per_frame": whole,
                  "horizontal_per_frame": stats(hs, n), "vertical_per_frame": stats(vs, n), "bytes_per_frame": moved // n,
                  "fraction_of_hbm_peak": round(moved / (whole["median_ms"] * n * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
                  "resize_nearest_per_frame_ms": near["median_ms"], "pillow_host_per_frame_ms": round(host_ms, 3)})
            with_f = stats(timed(torch, lambda: vp.process_frames(frames, dith, "regular", min(oh, ow), None, downscale_filter=name), max(2, R // 2)), n)
            without = stats(timed(torch, lambda: vp.process_frames(frames, dith, "regular", min(oh, ow), None), max(2, R // 2)), n)
            emit({"what": f"process_frames {label} {name} against NEAREST (Bayer 4x4, 16 colours, no enlargement)", "with_filter_per_frame": with_f,
                  "nearest_per_frame": without})
            staged.append((label, name, h, w, oh, ow))
            del plan
        del out
    # the A/B of the horizontal pass: the experiments library, alternating
    be.drop_resample_plans()
    prev = _lib.select(True)
    try:
        for label, name, h, w, oh, ow in staged:
            if shape != (h, w):
                del frames
                torch.cuda.empty_cache()
                frames, shape = image_like(torch, n, h, w), (h, w)
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
            plan = be.ResamplePlan(name, h, w, oh, ow)
            got = {"staged": [], "naive": []}
            for _ in range(3):
                for which in ("staged", "naive"):
                    os.environ["DP_RESAMPLE_H"] = which      # (staged: where the spans fit a staged row, the naive kernel otherwise)
                    got[which] += passes(be, torch, lambda: be.resample(frames, oh, ow, name, out=out, plan=plan), max(2, R // 2), warmup=1)[0]
            emit({"what": f"A/B horizontal pass {label} {name} (experiments library): the staged kernel against the naive one",
                  "staged_per_frame": stats(got["staged"], n), "naive_per_frame": stats(got["naive"], n)})
            del plan, out
    finally:
        os.environ.pop("DP_RESAMPLE_H", None)
        be.drop_resample_plans()
        _lib.select(prev)


if __name__ == "__main__":
    main()
