"""Wavelet dithering (wavelet.hip) on the GPU, timed with HIP events around backend.wavelet: one 1080p frame, one 4K frame
and a 24-frame 4K batch, haar and sym4 (filter length 8), 16 and 256 colours; the first call on a geometry (the random
stream is generated on the host with numpy and uploaded then) against a call on a cached geometry.
usage (repository root): python tools/bench_scripts/wavelet_time.py"""
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
    be.wavelet(x, P, params, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.wavelet(x, P, params, out=out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall_ms(x, P, params):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    be.wavelet(x, P, params)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


f1080 = torch.from_numpy(imgl(1080, 1920, 16)).cuda().unsqueeze(0)
f4k = torch.from_numpy(imgl(2160, 3840, 17)).cuda().unsqueeze(0)
b4k = f4k.repeat(24, 1, 1, 1).contiguous()
print("ms (median of 5, HIP events)   1080p     4K    24 x 4K (per frame)   4K first call / cached (wall)", flush=True)
for K in (16, 256):
    P = palette(K)
    for wavelet in ("haar", "sym4"):
        params = {"wavelet": wavelet}
        be._WL_STREAMS.clear()
        first = wall_ms(f4k, P, params)
        cached = wall_ms(f4k, P, params)
        one = time_ms(f1080, P, params)
        four = time_ms(f4k, P, params)
        many = time_ms(b4k, P, params, reps=3)
        print(f"  {K:4d} colours {wavelet:6s} {one:7.3f} {four:7.3f} {many:9.3f} ({many / 24:6.3f})      "
              f"{first:7.2f} / {cached:6.2f}", flush=True)
