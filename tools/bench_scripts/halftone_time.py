"""Halftone dithering (halftone.hip) on the GPU, timed with HIP events around backend.halftone: one 1080p frame, one 4K frame
and a 24-frame 4K batch, at the default parameters and on the pow path (dot_gain 1.5), 16 and 256 colours; the first call
on a geometry (pow path: the fix-up list is built then, one host round trip) against a call on a cached geometry.
usage (repository root): python tools/bench_scripts/halftone_time.py"""
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
from dither_pie_amd import backend as be
from dither_pie_amd.dithering_lib import prepare_palette
from oracle.oracle import imgl, palr


def palette(K):
    return be.Palette(*prepare_palette(palr(K, 7), False))


def time_ms(x, P, params, reps=5):
    out = torch.empty_like(x)
    be.halftone(x, P, params, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.halftone(x, P, params, out=out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def first_call_ms(x, P, params):
    be._HT_FIXUPS.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    be.halftone(x, P, params)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


f1080 = torch.from_numpy(imgl(1080, 1920, 16)).cuda().unsqueeze(0)
f4k = torch.from_numpy(imgl(2160, 3840, 17)).cuda().unsqueeze(0)
b4k = f4k.repeat(24, 1, 1, 1).contiguous()
SETS = (("default", {}), ("pow dot_gain=1.5", {"dot_gain": 1.5}))
print("ms (median of 5, HIP events)   1080p     4K    24 x 4K (per frame)   4K first call / cached (wall)", flush=True)
for K in (16, 256):
    P = palette(K)
    for name, params in SETS:
        first = first_call_ms(f4k, P, params)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        be.halftone(f4k, P, params)
        torch.cuda.synchronize()
        cached = (time.perf_counter() - t0) * 1e3
        one = time_ms(f1080, P, params)
        four = time_ms(f4k, P, params)
        many = time_ms(b4k, P, params, reps=3)
        print(f"  {K:4d} colours {name:18s} {one:7.3f} {four:7.3f} {many:9.3f} ({many / 24:6.3f})      "
              f"{first:7.2f} / {cached:6.2f}", flush=True)
