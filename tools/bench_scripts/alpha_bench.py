"""Times of the transparency layer on one MI355X (warm clocks; median [p10-p90]).

  python tools/bench_scripts/alpha_bench.py [--repeats 10] [--quick] [--out FILE]

  * dp_alpha_idiff_u8 against dp_idiff_u8 (Floyd-Steinberg and JJN) and dp_alpha_dotdiff_u8 against dp_dotdiff_u8 (Knuth's matrix) on 24
    resident image-like 1080p frames and on one 40 x 56 sprite, 16 colours, from the library's own HIP events (dp_profile_*): every
    masked call ALTERNATES with its unmasked counterpart on the same frames, for an all-opaque mask (the cost of the extra byte per
    pixel on the dependency chain) and for a half-masked one (random, 1/2);
  * the split / key / join kernels on the same frames against the bytes they move (8, 3 and 8 per pixel: the key reads a plane and
    a mask and writes a plane) as a share of the HBM peak (8 TB/s);
  * apply_dithering_png(image, alpha=AlphaMode()) end to end (host clock) against the same call without alpha, on a 1080p RGBA image
    and on the sprite.
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
PALETTE = [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 200, 30), (30, 30, 200), (220, 220, 40), (40, 220, 220), (220, 40, 220), (128, 128, 128),
           (64, 64, 64), (192, 192, 192), (128, 64, 0), (0, 128, 64), (64, 0, 128), (250, 150, 100), (100, 150, 250)]
KNUTH = ((34, 48, 40, 32, 29, 15, 23, 31), (42, 58, 56, 53, 21, 5, 7, 10), (50, 62, 61, 45, 13, 1, 2, 18), (38, 46, 54, 37, 25, 17, 9, 26),
         (28, 14, 22, 30, 35, 49, 41, 33), (20, 4, 6, 11, 43, 59, 57, 52), (12, 0, 3, 19, 51, 63, 60, 44), (24, 16, 8, 27, 39, 47, 55, 36))


def stats(ms, per=1):
    a = np.sort(np.asarray(ms, np.float64)) / per
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 5),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 5), "repeats": len(a)}


def image_like(torch, n, h, w):
    """Smooth gradients with grain and a few flat blocks: what a photo or a rendered sprite sheet looks like to a ditherer."""
    g = torch.Generator(device="cuda").manual_seed(3)
    y = torch.arange(h, device="cuda").view(h, 1).float()
    x = torch.arange(w, device="cuda").view(1, w).float()
    base = torch.stack([(x * (200.0 / w) + 20).expand(h, w), (y * (180.0 / h) + 30).expand(h, w), ((x + y) * (150.0 / (w + h)) + 40)], dim=-1)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for t in range(n):
        f = base + torch.randint(-12, 13, base.shape, device="cuda", generator=g).float() + 3.0 * t
        out[t] = f.clamp_(0, 255).to(torch.uint8)
    return out


def alternating(be, torch, fa, fb, repeats, warmup=2):
    """fa and fb in turn, `repeats` times each, timed by the library's own HIP events -> (times of fa, times of fb) in ms."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    be.profile_enable(True)
    be.profile_read()
    ta, tb = [], []
    for _ in range(repeats):
        for f, t in ((fa, ta), (fb, tb)):
            f()
            a, b, _ = be.profile_read()
            t.append(a + b)
    be.profile_enable(False)
    return ta, tb


def library_events(be, torch, fn, repeats, warmup=2):
    return alternating(be, torch, fn, fn, repeats, warmup)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small frames and 3 repeats: a rehearsal of the script, not a measurement")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from PIL import Image
    from dither_pie_amd import backend as be
    from dither_pie_amd import dithering_lib as dl
    if not torch.cuda.is_available():
        raise SystemExit("alpha_bench needs an MI355X: there is no CPU fallback and no CPU timing")
    repeats = 3 if args.quick else args.repeats
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    P = be.Palette(*dl.prepare_palette(PALETTE, False))
    P.pattern_prepare()
    kernels = dl.ErrorDiffusionKernel
    taps = {name: ([tuple(int(v) for v in t) for t in kernels.get_kernel(name)["weights"]], int(kernels.get_kernel(name)["divisor"]))
            for name in ("floyd_steinberg", "jjn")}
    classes = np.array(KNUTH, np.uint8)
    for label, n, (h, w) in (("1080p", N_FRAMES, (270, 480) if args.quick else (1080, 1920)), ("sprite", 1, (40, 56))):
        frames = image_like(torch, n, h, w)
        px = h * w
        out_a, out_b = torch.empty_like(frames), torch.empty_like(frames)
        g = torch.Generator(device="cuda").manual_seed(5)
        masks = {"all_opaque": torch.zeros((n, h, w), dtype=torch.uint8, device="cuda"),
                 "half_masked": torch.randint(0, 2, (n, h, w), device="cuda", generator=g).to(torch.uint8)}
        for mname, mask in masks.items():
            for tname, (tp, div) in taps.items():
                tm, tu = alternating(be, torch, lambda: be.idiff_masked(frames, mask, P, tp, div, 256, out=out_a),
                                     lambda: be.idiff(frames, P, tp, div, 256, out=out_b), repeats)
                emit(figure="idiff", frames=label, h=h, w=w, n=n, taps=tname, mask=mname, masked_per_frame=stats(tm, n), unmasked_per_frame=stats(tu, n),
                     ratio=round(float(np.median(tm) / np.median(tu)), 4))
            tm, tu = alternating(be, torch, lambda: be.dotdiff_masked(frames, mask, P, classes, 256, out=out_a),
                                 lambda: be.dotdiff(frames, P, classes, 256, out=out_b), repeats)
            emit(figure="dotdiff", frames=label, h=h, w=w, n=n, mask=mname, masked_per_frame=stats(tm, n), unmasked_per_frame=stats(tu, n),
                 ratio=round(float(np.median(tm) / np.median(tu)), 4))
        # split / key / join against the bytes they move
        rgba = torch.cat([frames, torch.randint(0, 256, (n, h, w, 1), device="cuda", generator=g).to(torch.uint8)], dim=-1).contiguous()
        planes = torch.randint(0, 16, (n, h, w), device="cuda", generator=g).to(torch.uint8)
        mask = masks["half_masked"]
        pout, jout = torch.empty_like(planes), torch.empty_like(rgba)
        for name, fn, nbytes in (("split_threshold", lambda: be.alpha_split(rgba), 8 * px * n),
                                 ("split_ordered_matte", lambda: be.alpha_split(rgba, "ordered", matrix=4, matte=(255, 255, 255)), 8 * px * n),
                                 ("key", lambda: be.alpha_key(planes, mask, 16, out=pout), 3 * px * n),
                                 ("join", lambda: be.alpha_join(frames, mask, (0, 0, 0), out=jout), 8 * px * n)):
            t = library_events(be, torch, fn, repeats)
            emit(figure=name, frames=label, h=h, w=w, n=n, per_frame=stats(t, n), bytes_per_call=nbytes,
                 hbm_peak_fraction=round(nbytes / (float(np.median(t)) * 1e-3) / HBM_PEAK_BYTES_PER_S, 4))
        # end to end: a PNG-8 with and without alpha (host clock, one image per call)
        image = Image.fromarray(rgba[0].cpu().numpy(), "RGBA")
        for dname, mode in (("bayer4x4", dl.DitherMode.BAYER), ("floyd_steinberg_int", dl.IntegerErrorDiffusionDitherStrategy())):
            d = dl.ImageDitherer(15, mode, list(PALETTE[:15]))

            def wall(fn):
                for _ in range(2):
                    fn()
                out = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    fn()
                    out.append((time.perf_counter() - t0) * 1e3)
                return out
            with_alpha = wall(lambda: d.apply_dithering_png(image, alpha=dl.AlphaMode()))
            without = wall(lambda: d.apply_dithering_png(image))
            emit(figure="apply_dithering_png", frames=label, h=h, w=w, dither=dname, with_alpha=stats(with_alpha), without_alpha=stats(without),
                 ratio=round(float(np.median(with_alpha) / np.median(without)), 4))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
