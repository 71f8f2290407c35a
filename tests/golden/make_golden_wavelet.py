#!/usr/bin/env python3
"""Record the wavelet fixtures from the REFERENCE itself (build container only).

Run with an interpreter that has the real PyWavelets (1.x) next to numpy 1.x and scipy, e.g.

    DITHER_PIE_REFERENCE=/path/to/dither_pie python3.9 tests/golden/make_golden_wavelet.py      (~1 minute)

Imports dobrosketchkun/dither_pie's dithering_lib unmodified -- with the real `pywt`, no stub -- and records, for seeded
synthetic inputs and palettes (formulas in oracle/oracle.py: rnd / grad / imgl / palr / generate_uniform_palette, plus
the flat and two-level images below), the outputs of
ImageDitherer(..., DitherMode.WAVELET, palette, use_gamma, params).apply_dithering and of WaveletDitherStrategy(**params)
.dither on non-integer float palettes.  pywt.dwt2 and the KD-tree are wrapped (not changed) to record what the reference
passes through them.  Only DATA is stored:
  wavelet.json  the cases (input / palette specs, parameters, use_gamma), the palettes used, the sha256 of every output,
                pywt's float32 filter taps of the nine wavelets read off its transforms with unit impulses, versions
  wavelet.npz   the full outputs of the cases of at most 64 x 64 pixels (and the 1 x N / N x 1 ones), the strategy-level
                outputs, the float32 reconstructions (the points of the k=2 query) of the cases of at most 2500 pixels and
                the float32 subbands of the cases of at most 300 pixels
"""
import hashlib
import json
import os
import sys
import time

import numpy as np
import pywt

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DITHER_PIE_REFERENCE", os.path.join(HERE, "..", "..", "..", "dither_pie"))

sys.path.insert(0, REF)
import dithering_lib as dl  # noqa: E402  (the reference)
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.oracle import generate_uniform_palette, grad, imgl, palr, rnd  # noqa: E402  (input formulas only)

WAVELETS = ["haar", "db1", "db2", "db4", "sym2", "sym4", "coif1", "bior1.3", "bior2.2"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_input(spec):
    kind = spec[0]
    if kind == "rnd":
        return rnd(spec[1], spec[2], spec[3])
    if kind == "grad":
        return grad(spec[1], spec[2])
    if kind == "imgl":
        return imgl(spec[1], spec[2], spec[3])
    if kind == "flat":  # one colour everywhere: every subband is constant, nothing is drawn before the thresholds
        return np.ascontiguousarray(np.broadcast_to(np.array(spec[3], np.uint8), (spec[1], spec[2], 3)))
    if kind == "flatch":  # imgl with channel spec[4] set to the constant spec[5]
        a = imgl(spec[1], spec[2], spec[3]).copy()
        a[..., spec[4]] = spec[5]
        return a
    if kind == "two":  # grey blocks of spec[3] and spec[4] in 8-pixel stripes
        y, x = np.mgrid[0:spec[1], 0:spec[2]]
        v = np.where(((x // 8) + (y // 8)) % 2 == 0, spec[3], spec[4]).astype(np.uint8)
        return np.ascontiguousarray(np.stack([v, v, v], -1))
    raise ValueError(spec)


def make_palette(spec):
    kind = spec[0]
    if kind == "none":
        return None
    if kind == "U":
        return generate_uniform_palette(spec[1])
    if kind == "palr":
        return palr(spec[1], spec[2] if len(spec) > 2 else 7)
    if kind == "dup":  # palr(K) followed by its first `n` entries again
        p = palr(spec[1], spec[3] if len(spec) > 3 else 7)
        return p + p[:spec[2]]
    if kind == "grey":  # greys 0, step, 2 step, ... (exact distance ties halfway between entries)
        return [(v, v, v) for v in range(0, 256, spec[1])]
    raise ValueError(spec)


def _case(name, pal, ncol, inp, gamma=False, **params):
    return (name, pal, ncol, inp, gamma, params)


# (name, palette spec, num_colors, input spec, use_gamma, params)
CASES = [
    # every wavelet, an odd size
    *[_case(f"wl_37x53_{w}", ("palr", 16), 16, ("imgl", 37, 53, 4), wavelet=w) for w in WAVELETS],
    # degenerate geometries: lines shorter than the filter
    _case("wl_1x1_p2", ("palr", 2), 2, ("rnd", 1, 1, 1)),
    _case("wl_1x1_db4", ("palr", 4), 4, ("rnd", 1, 1, 2), wavelet="db4"),
    _case("wl_1x200_p8", ("palr", 8), 8, ("rnd", 1, 200, 3)),
    _case("wl_1x77_sym4", ("palr", 8), 8, ("imgl", 1, 77, 4), wavelet="sym4"),
    _case("wl_200x1_p16_g", ("palr", 16), 16, ("rnd", 200, 1, 5), True),
    _case("wl_91x1_coif1", ("palr", 16), 16, ("imgl", 91, 1, 6), wavelet="coif1"),
    _case("wl_2x2_p4", ("palr", 4), 4, ("rnd", 2, 2, 7)),
    _case("wl_2x2_bior2.2", ("palr", 4), 4, ("rnd", 2, 2, 8), wavelet="bior2.2"),
    _case("wl_3x5_db4", ("palr", 8), 8, ("rnd", 3, 5, 9), wavelet="db4"),
    _case("wl_3x5_sym4", ("palr", 8), 8, ("rnd", 3, 5, 10), wavelet="sym4"),
    _case("wl_3x5_coif1", ("palr", 8), 8, ("rnd", 3, 5, 11), wavelet="coif1"),
    _case("wl_7x4_db2", ("palr", 8), 8, ("rnd", 7, 4, 12), wavelet="db2"),
    # Q
    _case("wl_64x64_q1", ("palr", 16), 16, ("imgl", 64, 64, 13), subband_quant=1),
    _case("wl_64x64_q2", ("palr", 16), 16, ("imgl", 64, 64, 14), subband_quant=2),
    _case("wl_64x64_q32_db4", ("palr", 16), 16, ("imgl", 64, 64, 15), wavelet="db4", subband_quant=32),
    _case("wl_64x64_q33_sym2", ("palr", 16), 16, ("imgl", 64, 64, 16), wavelet="sym2", subband_quant=33),
    _case("wl_64x64_q70000", ("palr", 16), 16, ("imgl", 64, 64, 17), subband_quant=70000),
    _case("wl_40x56_q3_bior1.3", ("palr", 16), 16, ("rnd", 40, 56, 18), wavelet="bior1.3", subband_quant=3),
    # seeds
    _case("wl_64x64_s0", ("palr", 16), 16, ("imgl", 64, 64, 19), seed=0),
    _case("wl_64x64_s9999_coif1", ("palr", 16), 16, ("imgl", 64, 64, 20), wavelet="coif1", seed=9999),
    _case("wl_64x64_s123456", ("palr", 16), 16, ("imgl", 64, 64, 21), seed=123456),
    _case("wl_64x64_s4294967295", ("palr", 16), 16, ("rnd", 64, 64, 22), wavelet="db2", seed=4294967295),
    # gamma, palette sizes
    _case("wl_64x64_p2_g", ("palr", 2, 11), 2, ("imgl", 64, 64, 23), True),
    _case("wl_64x64_p64_g_db4", ("palr", 64), 64, ("imgl", 64, 64, 24), True, wavelet="db4"),
    _case("wl_64x64_p256", ("palr", 256), 256, ("rnd", 64, 64, 25), wavelet="sym4"),
    _case("wl_64x64_p1024", ("palr", 1024), 1024, ("imgl", 64, 64, 26)),
    _case("wl_60x50_p1024_g", ("palr", 1024, 3), 1024, ("rnd", 60, 50, 27), True, wavelet="coif1"),
    _case("wl_dup_p17", ("dup", 12, 5), 17, ("imgl", 64, 64, 28)),
    _case("wl_mediancut_16", ("none",), 16, ("imgl", 64, 80, 29), wavelet="db2"),
    _case("wl_mediancut_64_g", ("none",), 64, ("imgl", 48, 72, 30), True),
    _case("wl_U27_grad", ("U", 27), 27, ("grad", 50, 61)),
    # flat images and channels (skipped subbands), exact ties
    _case("wl_flat_haar", ("palr", 16), 16, ("flat", 37, 53, (120, 64, 200))),
    _case("wl_flat_db4", ("palr", 16), 16, ("flat", 37, 53, (120, 64, 200)), wavelet="db4"),
    _case("wl_flat_sym4", ("palr", 16), 16, ("flat", 40, 40, (7, 250, 31)), wavelet="sym4"),
    _case("wl_flat_coif1", ("palr", 16), 16, ("flat", 33, 47, (99, 99, 99)), wavelet="coif1"),
    _case("wl_flat_bior2.2", ("palr", 16), 16, ("flat", 33, 47, (99, 99, 99)), wavelet="bior2.2"),
    _case("wl_flatch_g_haar", ("palr", 16), 16, ("flatch", 64, 64, 31, 1, 128)),
    _case("wl_flatch_b_db4", ("palr", 16), 16, ("flatch", 64, 64, 32, 2, 0), wavelet="db4"),
    _case("wl_flatch_r_coif1", ("palr", 16), 16, ("flatch", 64, 64, 33, 0, 255), wavelet="coif1"),
    _case("wl_tie_grey10_flat", ("grey", 10), 26, ("flat", 40, 40, (5, 5, 5))),
    _case("wl_tie_grey10_two", ("grey", 10), 26, ("two", 48, 64, 15, 45)),
    _case("wl_tie_grey64_two_db2", ("grey", 64), 4, ("two", 48, 64, 32, 96), wavelet="db2"),
    _case("wl_tie_grey10_two_bior2.2", ("grey", 10), 26, ("two", 64, 48, 25, 125), wavelet="bior2.2"),
    # larger
    _case("wl_121x203_p256_sym4", ("palr", 256), 256, ("rnd", 121, 203, 34), wavelet="sym4"),
    _case("wl_121x203_p16_g_coif1", ("palr", 16), 16, ("imgl", 121, 203, 35), True, wavelet="coif1", subband_quant=5),
    _case("wl_300x300_p32_db4", ("palr", 32), 32, ("imgl", 300, 300, 36), wavelet="db4"),
    _case("wl_1080x1920_p8", ("palr", 8), 8, ("imgl", 1080, 1920, 37)),
    _case("wl_1080x1920_p16_db4", ("palr", 16), 16, ("imgl", 1080, 1920, 38), wavelet="db4"),
    _case("wl_1080x1920_p256_sym4_g", ("palr", 256), 256, ("imgl", 1080, 1920, 39), True, wavelet="sym4"),
    _case("wl_2160x3840_p16", ("palr", 16), 16, ("imgl", 2160, 3840, 40)),
]

# WaveletDitherStrategy(**params).dither(pixels f32, palette f32 (non-integer values), (h, w))
STRATEGY_CASES = [
    ("st_40x56_K5", 5, ("rnd", 40, 56, 50), {}),
    ("st_40x56_K40_db4", 40, ("imgl", 40, 56, 51), {"wavelet": "db4", "subband_quant": 4, "seed": 7}),
    ("st_33x47_K300_coif1", 300, ("rnd", 33, 47, 52), {"wavelet": "coif1", "subband_quant": 16}),
]


def impulse_taps(name):
    """pywt's float32 filters, read off its float32 transforms with unit impulses (0 + f * 1 = f exactly)."""
    w = pywt.Wavelet(name)
    F = w.dec_len
    res = {}
    N = 4 * F + 8
    o = N // 4
    for key, which in (("dec_lo", 0), ("dec_hi", 1)):
        t = np.zeros(F, np.float32)
        for m in range(F):
            x = np.zeros(N, np.float32)
            x[2 * o + 1 - m] = 1
            t[m] = pywt.dwt(x, w, mode="symmetric")[which][o]
        res[key] = t
    n = 2 * F + 4
    oi = n // 2
    for key, which in (("rec_lo", 0), ("rec_hi", 1)):
        t = np.zeros(F, np.float32)
        for m in range(F):
            a = np.zeros(n, np.float32)
            a[F // 2 - 1 + oi - m // 2] = 1
            z = np.zeros(n, np.float32)
            r = pywt.idwt(a, z, w, mode="symmetric") if which == 0 else pywt.idwt(z, a, w, mode="symmetric")
            assert r.dtype == np.float32
            t[m] = r[2 * oi + m % 2]
        res[key] = t
    return res


class _Recorder:
    """Wraps the reference's module-level pywt.dwt2 and KDTree: passes every call through unchanged and keeps what the
    reference hands them (the subbands of each channel, the points of the k=2 query)."""

    def __init__(self):
        self.subbands, self.points = [], None
        self._dwt2, self._kdtree = dl.pywt.dwt2, dl.KDTree
        rec = self

        class KD(self._kdtree):
            def query(self, x, *a, **k):
                rec.points = np.array(x, copy=True)
                return super().query(x, *a, **k)

        def dwt2(*a, **k):
            out = rec._dwt2(*a, **k)
            rec.subbands.append([np.array(out[0])] + [np.array(c) for c in out[1]])
            return out

        self.KD, self.dwt2 = KD, dwt2

    def __enter__(self):
        dl.pywt.dwt2, dl.KDTree = self.dwt2, self.KD
        return self

    def __exit__(self, *exc):
        dl.pywt.dwt2, dl.KDTree = self._dwt2, self._kdtree


def main():
    import PIL
    import scipy
    out = {"versions": {"numpy": np.__version__, "scipy": scipy.__version__, "pillow": PIL.__version__,
                        "pywt": pywt.__version__, "python": sys.version.split()[0]},
           "taps": {}, "cases": [], "strategy": []}
    for w in WAVELETS:
        out["taps"][w] = {k: [float(v) for v in t] for k, t in impulse_taps(w).items()}
    npz = {}
    for name, pspec, ncol, ispec, gamma, params in CASES:
        t0 = time.time()
        arr = make_input(ispec)
        pal = make_palette(pspec)
        d = dl.ImageDitherer(ncol, dl.DitherMode.WAVELET, None if pal is None else list(pal), gamma, dict(params))
        with _Recorder() as rec:
            res = np.array(d.apply_dithering(Image.fromarray(arr)))
        used = [list(map(int, c)) for c in d.palette]
        h, w = arr.shape[:2]
        case = {"name": name, "palette_spec": list(pspec), "num_colors": ncol, "input": list(ispec), "use_gamma": gamma,
                "params": params, "h": int(h), "w": int(w), "palette": used,
                "input_sha256": sha(arr), "output_sha256": sha(res), "points_sha256": sha(rec.points.astype(np.float32))}
        if h * w <= 64 * 64 or h == 1 or w == 1:
            npz["out_" + name] = res
            case["full"] = True
        if h * w <= 2500:
            npz["rec_" + name] = rec.points.astype(np.float32).reshape(h, w, 3)
            case["rec"] = True
        if h * w <= 300:
            for ch, sbs in enumerate(rec.subbands):
                for s, sb in zip("AHVD", sbs):
                    assert sb.dtype == np.float32
                    npz[f"sb_{name}_{ch}{s}"] = sb
            case["subbands"] = True
        out["cases"].append(case)
        print(f"{name}: {time.time() - t0:.2f} s {case['output_sha256'][:16]}", flush=True)
    for name, K, ispec, params in STRATEGY_CASES:
        arr = make_input(ispec)
        h, w, _ = arr.shape
        pal = (np.random.RandomState(K).rand(K, 3) * 255.0).astype(np.float32)
        res = dl.WaveletDitherStrategy(**params).dither(arr.reshape(-1, 3).astype(np.float32), pal, (h, w))
        npz["st_pal_" + name] = pal
        npz["st_out_" + name] = np.asarray(res)
        out["strategy"].append({"name": name, "K": K, "input": list(ispec), "params": params,
                                "output_sha256": sha(np.asarray(res))})
    with open(os.path.join(HERE, "wavelet.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    np.savez_compressed(os.path.join(HERE, "wavelet.npz"), **npz)


if __name__ == "__main__":
    main()
