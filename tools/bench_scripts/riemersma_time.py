"""Riemersma dithering (riemersma.hip) on the GPU, timed with HIP events around backend.riemersma: one 1080p frame and a batch of
64 such frames at 16 / 64 / 256 / 1024 colours, then ns per in-image path step at 1024 x 1024 (every path index in the image) and
1080 x 1080 (dim 2048: 72 % of the path off the image -- equal cost per step shows the off-image squares skipped).
usage (repository root): python tools/bench_scripts/riemersma_time.py"""
import sys
sys.path.insert(0, '.')
import numpy as np
import torch
from dither_pie_amd import backend as be
from dither_pie_amd.dithering_lib import prepare_palette
from oracle.oracle import imgl, palr


def palette(K):
    return be.Palette(*prepare_palette(palr(K, 7), False))


def time_ms(x, P, reps=3):
    out = torch.empty_like(x)
    be.riemersma(x, P, out=out)   # first call
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.riemersma(x, P, out=out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


frame = torch.from_numpy(imgl(1080, 1920, 16)).cuda().unsqueeze(0)
batch = frame.repeat(64, 1, 1, 1).contiguous()
print("1080 x 1920           one frame ms   64-frame batch ms (per frame)", flush=True)
for K in (16, 64, 256, 1024):
    P = palette(K)
    one = time_ms(frame, P)
    many = time_ms(batch, P, reps=2)
    print(f"  {K:5d} colours      {one:10.1f}      {many:10.1f} ({many / 64:7.2f})", flush=True)
print("ns per in-image step", flush=True)
for K in (16, 256):
    P = palette(K)
    for h, w in ((1024, 1024), (1080, 1080)):
        x = torch.from_numpy(imgl(h, w, 5)).cuda().unsqueeze(0)
        ms = time_ms(x, P)
        print(f"  {K:5d} colours {h} x {w}: {ms * 1e6 / (h * w):7.1f} ns  ({ms:.1f} ms)", flush=True)
