"""Times and file sizes of the temporal hold on one MI355X (warm clocks; median [p10-p90]).

  python tools/bench_scripts/hold_bench.py [--repeats 10] [--quick] [--out FILE]

  * dp_hold_u8 (cell 8, tol 4, share 1/16: the defaults) on 24 resident 1080p frames and on 24 resident 64 x 114 frames (what
    pixelization at max_size 64 makes of them): per frame, from events around the call and from the library's own HIP events
    (dp_profile_*); 5 bytes per pixel and frame (3 source, 1 fresh index, 1 output) plus 8 bytes per pixel of state per call (4
    read, 4 written) over the call's time as a fraction of the HBM peak (8 TB/s);
  * beside it, in the same process on the same planes: dp_index_delta_u8 (2 bytes per pixel and frame: the comparison point for a
    pass of this shape) and the dither that produced the planes (integer Floyd-Steinberg and Bayer 4x4, 16 colours);
  * a synthetic clip (a static image with grain of +-2, one moving block; 24 frames of 270 x 480): the bytes of the GIF that
    process_video_gif writes for it with delta=True (process_frames_indexed into gif.GifWriter), with and without the hold, for both
    dithers, and the pixels the hold refreshed.
Run from the root of the tree; prints one JSON line per figure.  Every figure is one run on one machine."""
import argparse
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES = 24
HBM_PEAK_BYTES_PER_S = 8.0e12
HOLD = (8, 4, 1 / 16)
PALETTE = [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 200, 30), (30, 30, 200), (220, 220, 40), (40, 220, 220), (220, 40, 220), (128, 128, 128),
           (64, 64, 64), (192, 192, 192), (128, 64, 0), (0, 128, 64), (64, 0, 128), (250, 150, 100), (100, 150, 250)]


def stats(ms, per=1):
    a = np.sort(np.asarray(ms, np.float64)) / per
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 5),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 5), "repeats": len(a)}


def clip(torch, n, h, w):
    """A static smooth image with grain of +-2 per channel and one block (an eighth of the height) that moves and changes."""
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.arange(h, device="cuda").view(h, 1).float()
    x = torch.arange(w, device="cuda").view(1, w).float()
    base = torch.stack([(x * (200.0 / w) + 20).expand(h, w), (y * (180.0 / h) + 30).expand(h, w), ((x + y) * (150.0 / (w + h)) + 40)], dim=-1)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    b = max(4, h // 8)
    for t in range(n):
        f = base + torch.randint(-2, 3, base.shape, device="cuda", generator=g).float()
        y0, x0 = (h // 4 + t * max(1, b // 6)) % (h - b), (w // 2 + t * max(1, b // 4)) % (w - b)
        f[y0:y0 + b, x0:x0 + b] = torch.randint(0, 256, (b, b, 3), device="cuda", generator=g).float()
        out[t] = f.clamp_(0, 255).to(torch.uint8)
    return out


def timed(torch, fn, repeats, warmup=2):
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


def library_events(be, torch, fn, repeats):
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


def ditherers():
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer, IntegerErrorDiffusionDitherStrategy
    return {"floyd_steinberg_int": ImageDitherer(16, IntegerErrorDiffusionDitherStrategy("floyd_steinberg"), list(PALETTE)),
            "bayer4x4": ImageDitherer(16, DitherMode.BAYER, list(PALETTE), dither_params={"size": "4x4"})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="small frames and 3 repeats: a rehearsal of the script, not a measurement")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import backend as be
    from dither_pie_amd.gif import GifWriter
    from dither_pie_amd.video_processor import process_frames_indexed
    if not torch.cuda.is_available():
        raise SystemExit("hold_bench needs an MI355X: there is no CPU fallback and no CPU timing")
    repeats = 3 if args.quick else args.repeats
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    cell, tol, share = HOLD
    share256 = int(round(share * 256))
    for label, (h, w) in (("1080p", (270, 480) if args.quick else (1080, 1920)), ("64x114", (64, 114))):
        frames = clip(torch, N_FRAMES, h, w)
        px = h * w
        for name, d in ditherers().items():
            planes, _ = d.apply_dithering_frames_indexed(frames)
            out = torch.empty_like(planes)
            state = [None]

            def run_hold():
                state[0] = be.hold(frames, planes, state[0], cell, tol, share256, out=out)[2]
            prev = torch.zeros(px, dtype=torch.uint8, device="cuda")
            dout = torch.empty_like(planes)
            t_hold = timed(torch, run_hold, repeats)
            t_lib = library_events(be, torch, run_hold, repeats)
            t_delta = timed(torch, lambda: be.index_delta(planes, prev, 16, out=dout), repeats)
            t_dither = timed(torch, lambda: d.apply_dithering_frames_indexed(frames), repeats)
            nbytes = N_FRAMES * px * 5 + 8 * px
            med = float(np.median(t_hold)) * 1e-3
            emit(figure="hold", frames=label, h=h, w=w, n=N_FRAMES, dither=name, cell=cell, tol=tol, share256=share256,
                 per_frame=stats(t_hold, N_FRAMES), per_frame_library_events=stats(t_lib, N_FRAMES), bytes_per_call=nbytes,
                 hbm_peak_fraction=round(nbytes / med / HBM_PEAK_BYTES_PER_S, 4), index_delta_per_frame=stats(t_delta, N_FRAMES),
                 dither_per_frame=stats(t_dither, N_FRAMES))
    # file sizes
    h, w = (68, 120) if args.quick else (270, 480)
    frames = clip(torch, N_FRAMES, h, w)
    for name, d in ditherers().items():
        sizes, refreshed = {}, None
        for held in (False, True):
            stream = be.HoldStream(cell=cell, tol=tol, share=share) if held else None
            buf = io.BytesIO()
            with GifWriter(buf, w, h, 25) as g:
                for a in range(0, N_FRAMES, 8):                                  # three batches, as the video path feeds them
                    planes, colours = process_frames_indexed(frames[a:a + 8], d, hold=stream)
                    g.add(planes, colours, True)
            sizes[held] = len(buf.getvalue())
        _, counts, _ = be.hold(frames, d.apply_dithering_frames_indexed(frames)[0], None, cell, tol, share256)
        refreshed = counts.cpu().numpy()
        emit(figure="gif_bytes", h=h, w=w, n=N_FRAMES, dither=name, delta=True, plain_bytes=sizes[False], held_bytes=sizes[True],
             ratio=round(sizes[True] / sizes[False], 4), refreshed_share_after_frame_0=round(float(refreshed[1:].mean()) / (h * w), 4))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
