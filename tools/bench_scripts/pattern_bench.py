"""Times of pattern (Knoll) dithering on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/pattern_bench.py [--repeats 10] [--quick]

  * the build of the 2^24-entry search table (dp_pattern_prepare, synchronous: host clock around it, and the sum of the
    nearest-only kernels inside it from the library's events) for a 16- and a 256-colour palette, integer and gamma;
  * dp_pattern_u8 per frame on 24 resident frames: 1080p m = 4 / 16 colours, 1080p m = 8 / 256 colours, 4K m = 8 / 256
    colours, on image-like content (smooth ramps with grain) -- with the table in 4 x 4 x 4 bricks and in plain
    r | g<<8 | b<<16 order (DP_PATTERN_PLAIN, experiments build), alternating, same session;
  * beside each: n = m * m times the nearest-only kernel (accelerator built) on the same batch and palette -- what the n
    searches would cost with what the library had before the table.  A ratio >= 1 means the table bought nothing.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import json
import os
import sys
import time

os.environ["DITHER_PIE_EXPERIMENTS"] = "1"          # the twin library: the only build that reads DP_PATTERN_PLAIN

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device (as tools/bench_scripts/scene_time.py)."""
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


def make_palette(be, dl, k, gamma, plain):
    rs = np.random.RandomState(5 + k)
    pal = [tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()]
    if plain:
        os.environ["DP_PATTERN_PLAIN"] = "1"
    else:
        os.environ.pop("DP_PATTERN_PLAIN", None)
    return be.Palette(*dl.prepare_palette(pal, gamma))


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
    for k, gamma in ((16, False), (256, False), (16, True), (256, True)):
        wall, kern = [], []
        for i in range(3):
            P = make_palette(be, dl, k, gamma, plain=False)
            torch.cuda.synchronize()
            be.profile_enable(True)
            be.profile_read()
            t = time.perf_counter()
            P.pattern_prepare()
            wall.append((time.perf_counter() - t) * 1e3)
            a, b, _ = be.profile_read()
            be.profile_enable(False)
            kern.append(a + b)
            del P
        print(json.dumps({"what": f"dp_pattern_prepare, {k} colours, gamma {gamma}", "wall_ms_runs": [round(v, 3) for v in wall],
                          "nearest_only_kernels_ms_runs": [round(v, 3) for v in kern]}), flush=True)

    # ---- the kernel, both layouts, and n x nearest-only
    cases = [("1080p", 1080, 1920, 4, 16), ("1080p", 1080, 1920, 8, 256), ("4K", 2160, 3840, 8, 256)]
    if args.quick:
        cases = [("tiny", 67, 129, 4, 16), ("tiny", 67, 129, 8, 256)]
    for name, h, w, m, k in cases:
        frames = image_like(torch, N_FRAMES, h, w)
        out = torch.empty_like(frames)
        pals = {"brick": make_palette(be, dl, k, False, plain=False)}
        pals["brick"].pattern_prepare()
        pals["plain"] = make_palette(be, dl, k, False, plain=True)
        pals["plain"].pattern_prepare()
        os.environ.pop("DP_PATTERN_PLAIN", None)
        res = {"brick": [], "plain": []}
        for layout in ("brick", "plain", "brick", "plain"):             # alternating
            res[layout] += profiled(be, torch, lambda: be.pattern(frames, pals[layout], m, 128, out=out), R)
        assert torch.equal(be.pattern(frames, pals["brick"], m, 128), be.pattern(frames, pals["plain"], m, 128))
        pals["brick"].build_accel()
        near = profiled(be, torch, lambda: be.ordered(frames, pals["brick"], be.MODE_NEAREST, out=out), R)
        near_ms = float(np.median(near)) / N_FRAMES
        rec = {"what": f"dp_pattern_u8 {name} m={m} {k} colours, 24 frames, image-like, strength 128", "n": m * m,
               "nearest_only_ms_per_frame": round(near_ms, 4), "n_x_nearest_only_ms_per_frame": round(m * m * near_ms, 4)}
        for layout in ("brick", "plain"):
            s = stats(res[layout])
            per = s["median_ms"] / N_FRAMES
            rec[layout] = {"ms_per_frame": round(per, 4), "p10": round(s["p10_ms"] / N_FRAMES, 4), "p90": round(s["p90_ms"] / N_FRAMES, 4),
                           "repeats": s["repeats"], "ratio_to_n_x_nearest_only": round(per / (m * m * near_ms), 4)}
        print(json.dumps(rec), flush=True)
        del frames, out, pals
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
