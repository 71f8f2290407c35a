"""The numpy statement of include/ditherpie_hip_resample.h: Pillow's Image.resize for RGB uint8 frames with the BOX, BILINEAR,
HAMMING, BICUBIC and LANCZOS filters, bit for bit (tests/test_resample_cpu.py holds it against Pillow itself; where the two
ever disagree, Pillow wins and this file is corrected).

Coefficients of one axis (Pillow's precompute_coeffs + normalize_coeffs_8bpc, whole source extent): Python floats are float64
and every operation below is one rounded operation in the header's order; sin and cos are math's, i.e. the C library's, as in
Pillow and in csrc/host_logic.h.  Everything after the coefficients is integer."""
import math

import numpy as np

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")          # DP_RESAMPLE_* order
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
BITS = 22
MAX_SIZE = 16384


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        x = abs(x)
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))
    if name == "bicubic":
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(name)


def coeffs(n_in, n_out, name):
    """-> (ksize, bounds int32 [n_out, 2] = (first source position, count), k int32 [n_out, ksize], zeros behind the count)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = SUPPORT[name] * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(sup)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)                           # int() truncates toward zero, as the C cast does
        xmax = min(int(center + sup + 0.5), n_in) - xmin
        w = [weight(name, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, k


def one_pass(src, bounds, k, axis, shift=0):
    """One pass along `axis` of an [..] uint8 array: clamp((2^21 + sum src[xmin + x] * k[x]) >> 22, 0, 255) in int64 (a plan's sums
    fit int32), -> uint8."""
    src = np.moveaxis(np.asarray(src), axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for xx, (xmin, cnt) in enumerate(bounds.tolist()):
        xmin -= shift
        kk = k[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (src.ndim - 1))
        s = (1 << (BITS - 1)) + (src[xmin:xmin + cnt] * kk).sum(axis=0)
        out[xx] = np.clip(s >> BITS, 0, 255)                             # >> of a numpy int64 is arithmetic: it floors
    return np.moveaxis(out, 0, axis)


def plan(name, h, w, oh, ow):
    """What the resize does, in Pillow's order: the vertical coefficients first, the source rows y0 .. y1-1 they read, then which
    passes run.  -> dict(ver=(ksize, bounds, k), hor=... or None, y0, y1, need_h, need_v)."""
    if name not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}")
    if not all(isinstance(v, (int, np.integer)) and 1 <= v <= MAX_SIZE for v in (h, w, oh, ow)) or h * w > 1 << 30:
        raise ValueError(f"sizes must lie in 1 .. {MAX_SIZE} with h * w <= 2^30")
    ver = coeffs(h, oh, name)
    y0 = int(ver[1][0, 0])
    y1 = int(ver[1][-1, 0] + ver[1][-1, 1])
    need_h, need_v = ow != w, oh != h
    return dict(ver=ver, hor=coeffs(w, ow, name) if need_h else None, y0=y0, y1=y1, need_h=need_h, need_v=need_v)


def resample(frames, oh, ow, name):
    """[N, H, W, 3] or [H, W, 3] uint8 -> the same with H, W = oh, ow."""
    f = np.asarray(frames)
    if f.dtype != np.uint8 or f.ndim not in (3, 4) or f.shape[-1] != 3:
        raise ValueError("frames must be [N, H, W, 3] or [H, W, 3] uint8")
    x = f[None] if f.ndim == 3 else f
    p = plan(name, x.shape[1], x.shape[2], oh, ow)
    shift = 0
    if p["need_h"]:
        if p["need_v"]:
            x = x[:, p["y0"]:p["y1"]]                                    # the uint8 intermediate has these rows only
            shift = p["y0"]
        x = one_pass(x, p["hor"][1], p["hor"][2], 2)
    if p["need_v"]:
        x = one_pass(x, p["ver"][1], p["ver"][2], 1, shift)
    x = np.ascontiguousarray(x).copy() if not (p["need_h"] or p["need_v"]) else np.ascontiguousarray(x)
    return x[0] if f.ndim == 3 else x


def plan_sums(name, h, w, oh, ow):
    """-> (max |k|, max over the output positions of 255 * sum |k| + 2^21) over the passes that run: what the planner records."""
    p = plan(name, h, w, oh, ow)
    big, need = 0, 0
    for axis, on in (("ver", p["need_v"]), ("hor", p["need_h"])):
        if on:
            k = np.abs(p[axis][2].astype(np.int64))
            big = max(big, int(k.max()))
            need = max(need, int(255 * k.sum(axis=1).max() + (1 << (BITS - 1))))
    return big, need


def workspace_bytes(name, n, h, w, oh, ow):
    p = plan(name, h, w, oh, ow)
    if n < 1 or not (p["need_h"] and p["need_v"]):
        return 0
    return (n * (p["y1"] - p["y0"]) * ow * 3 + 15) // 16 * 16


# the sweep of tests/test_resample_cpu.py: (h, w, oh, ow)
GEOMETRIES = [(37, 53, 8, 10), (17, 23, 40, 50), (24, 31, 24, 9), (29, 18, 7, 18), (8, 8, 1, 1), (5, 300, 5, 7), (33, 2, 3, 5),
              (130, 70, 66, 35), (21, 19, 21, 19)]
CONTENTS = ("noise", "extremes", "ramp")


def content(kind, n, h, w, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    if kind == "extremes":                                               # pure 0 / 255: BICUBIC and LANCZOS overshoot, the clamp works at both ends
        return (rs.randint(0, 2, (n, h, w, 3)) * 255).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        f = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], -1).astype(np.uint8)
        return np.stack([np.roll(f, i, axis=1) for i in range(n)])
    raise ValueError(kind)
