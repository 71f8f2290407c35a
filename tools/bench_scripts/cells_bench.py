"""Times of cell-palette dithering on one MI355X (the library's HIP events: dp_profile_*; warm clocks; median [p10-p90]).

  python tools/bench_scripts/cells_bench.py [--repeats 10] [--quick]

  * dp_cells_u8 on ONE frame per call and per frame of 24 resident frames, 1080p and 4K, on image-like content (smooth
    ramps with grain), for five settings: 8 x 8 cells with 2 of 16 colours (120 candidates per cell), 8 x 8 with 4 of 16
    (1820), 16 x 16 with 4 colours from one of four overlapping groups of eight (280) or of all sixteen (7280, the most a
    call can ask for), and the ZX Spectrum preset (8 x 8, 2 of 15 in two groups, 56);
  * beside each, in the same process on the same batch and palette: one pass of the nearest-only kernel (DP_MODE_NEAREST of
    dp_ordered_u8, accelerator built) -- the cost of constraining colour by the frame's palette alone, as context.
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

    S = dl.CellPaletteDitherStrategy
    rs = np.random.RandomState(21)
    pal16 = [tuple(c) for c in rs.randint(0, 256, (16, 3)).tolist()]
    # name, palette, cell, colours, fixed mask, groups
    settings = [("8x8 k=2 K=16", pal16, (8, 8), 2, 0, None),
                ("8x8 k=4 K=16", pal16, (8, 8), 4, 0, None),
                ("16x16 k=4 K=16 four groups of 8", pal16, (16, 16), 4, 0, [0x00FF, 0x0FF0, 0xFF00, 0xF00F]),
                ("16x16 k=4 K=16 four groups of 16 (the maximum)", pal16, (16, 16), 4, 0, [0xFFFF] * 4),
                ("ZX Spectrum preset", S.ZX_SPECTRUM_PALETTE, (8, 8), 2, 0, [0x00FF, 0x7F01])]
    sizes = [("1080p", 1080, 1920), ("4K", 2160, 3840)]
    if args.quick:
        sizes = [("tiny", 147, 197)]
    for size, h, w in sizes:
        frames = image_like(torch, N_FRAMES, h, w)
        out = torch.empty_like(frames)
        one_in, one_out = frames[:1].clone(), torch.empty_like(frames[:1])
        for name, pal, cell, k, fixed, groups in settings:
            P = be.Palette(*dl.prepare_palette(pal, False))
            kw = dict(fixed_mask=fixed, groups=groups)
            n_cand = be.cell_candidates(P.K, k, fixed, groups)
            one = stats(profiled(be, torch, lambda: be.cells(one_in, P, cell, k, 4, 64, out=one_out, **kw), R))
            batch = stats(profiled(be, torch, lambda: be.cells(frames, P, cell, k, 4, 64, out=out, **kw), R))
            P.build_accel()
            near_one = stats(profiled(be, torch, lambda: be.ordered(one_in, P, be.MODE_NEAREST, out=one_out), R))["median_ms"]
            near = float(np.median(profiled(be, torch, lambda: be.ordered(frames, P, be.MODE_NEAREST, out=out), R))) / N_FRAMES
            per = batch["median_ms"] / N_FRAMES
            print(json.dumps({
                "what": f"dp_cells_u8 {size}, {name}, matrix 4, spread 64, image-like", "candidates_per_cell": n_cand,
                "one_frame_per_call": {"cells_ms": one["median_ms"], "p10": one["p10_ms"], "p90": one["p90_ms"], "repeats": one["repeats"],
                                       "nearest_only_ms": near_one},
                "batch_of_24": {"ms_per_frame": round(per, 4), "p10": round(batch["p10_ms"] / N_FRAMES, 4),
                                "p90": round(batch["p90_ms"] / N_FRAMES, 4), "repeats": batch["repeats"],
                                "nearest_only_ms_per_frame": round(near, 4), "ratio_to_nearest_only": round(per / near, 1)}}), flush=True)
            del P
        del frames, out, one_in, one_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
