#!/usr/bin/env python3
"""Record the halftone fixtures from the REFERENCE itself (build container only).

Run:  python tests/golden/make_golden_halftone.py      (needs the reference checkout; ~1 minute)

Imports dobrosketchkun/dither_pie's dithering_lib the way make_golden.py does (an in-memory stub stands in for the unused
`pywt` import; DITHER_PIE_REFERENCE names the checkout) and records, for seeded synthetic inputs and palettes (formulas
in oracle/oracle.py: rnd / grad / imgl / palr / generate_uniform_palette, plus "tiegrey" below), the outputs of
ImageDitherer(..., DitherMode.HALFTONE, palette, use_gamma, params).apply_dithering, of
HalftoneDitherStrategy(**params).dither on non-integer float palettes, and of _generate_halftone_screen_with_cells.
Only DATA is stored:
  halftone.json  the cases (input / palette specs, parameters, use_gamma), the palettes used, the sha256 of every output,
                 versions
  halftone.npz   the full outputs of the cases of at most 64 x 64 pixels (and the 1 x N / N x 1 ones), the strategy-level
                 outputs, and the screens / cell ids of the small geometries
"""
import hashlib
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DITHER_PIE_REFERENCE", os.path.join(HERE, "..", "..", "..", "dither_pie"))

sys.modules.setdefault("pywt", types.ModuleType("pywt"))
sys.path.insert(0, REF)
import dithering_lib as dl  # noqa: E402  (the reference)
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.oracle import generate_uniform_palette, grad, imgl, palr, rnd  # noqa: E402  (input formulas only)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_input(spec):
    kind = spec[0]
    if kind == "rnd":
        return rnd(spec[1], spec[2], spec[3])
    if kind == "grad":
        return grad(spec[1], spec[2])
    if kind == "grey":  # the first channel of grad() on all three: a grey ramp
        return np.ascontiguousarray(grad(spec[1], spec[2])[..., [0, 0, 0]])
    if kind == "imgl":
        return imgl(spec[1], spec[2], spec[3])
    if kind == "tiegrey":  # flat grey blocks at 5 + 10 k: with the "grey10" palette every interior cell mean is an exact tie
        y, x = np.mgrid[0:spec[1], 0:spec[2]]
        v = 5 + 10 * ((x // 24 + 3 * (y // 24)) % 25)
        return np.ascontiguousarray(np.stack([v, v, v], -1).astype(np.uint8))
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
    if kind == "grey10":  # greys 0, 10, ..., 250 (26 entries: more than one KD-tree leaf)
        return [(10 * i, 10 * i, 10 * i) for i in range(26)]
    raise ValueError(spec)


# (name, palette spec, num_colors, input spec, use_gamma, params)
CASES = [
    ("ht_1x1_p2", ("palr", 2), 2, ("rnd", 1, 1, 1), False, {}),
    ("ht_1x200_p8_cs3", ("palr", 8), 8, ("rnd", 1, 200, 2), False, {"cell_size": 3}),
    ("ht_200x1_p16_g", ("palr", 16), 16, ("rnd", 200, 1, 3), True, {}),
    ("ht_37x53_p16", ("palr", 16), 16, ("imgl", 37, 53, 4), False, {}),
    ("ht_37x53_p16_g", ("palr", 16), 16, ("imgl", 37, 53, 4), True, {}),
    ("ht_64x64_cs2", ("palr", 16), 16, ("imgl", 64, 64, 5), False, {"cell_size": 2}),
    ("ht_64x64_cs3_a15", ("palr", 16), 16, ("rnd", 64, 64, 6), False, {"cell_size": 3, "angle": 15.0}),
    ("ht_64x64_cs7.5_a37.5", ("palr", 32), 32, ("imgl", 64, 64, 7), False, {"cell_size": 7.5, "angle": 37.5}),
    ("ht_64x64_cs13_a90", ("palr", 16), 16, ("grad", 64, 64), False, {"cell_size": 13, "angle": 90.0}),
    ("ht_64x64_cs32_a0", ("palr", 16), 16, ("imgl", 64, 64, 8), True, {"cell_size": 32, "angle": 0.0}),
    ("ht_63x65_a135_square", ("palr", 16), 16, ("imgl", 63, 65, 9), False, {"angle": 135.0, "shape": "square"}),
    ("ht_63x65_am30_diamond", ("palr", 16), 16, ("imgl", 63, 65, 10), False, {"angle": -30.0, "shape": "diamond"}),
    ("ht_64x64_dg0.5", ("palr", 16), 16, ("imgl", 64, 64, 11), False, {"dot_gain": 0.5}),
    ("ht_64x64_dg1.5", ("palr", 16), 16, ("imgl", 64, 64, 12), False, {"dot_gain": 1.5}),
    ("ht_64x64_dg2", ("palr", 16), 16, ("imgl", 64, 64, 13), False, {"dot_gain": 2.0}),
    ("ht_64x64_dg3_g", ("palr", 16), 16, ("imgl", 64, 64, 14), True, {"dot_gain": 3.0}),
    ("ht_64x64_dots", ("palr", 16), 16, ("imgl", 64, 64, 15), False, {"min_dot_size": 0.2, "max_dot_size": 0.65}),
    ("ht_64x64_dots_sq", ("palr", 16), 16, ("imgl", 64, 64, 16), False,
     {"min_dot_size": 0.5, "max_dot_size": 0.5, "shape": "square", "sharpness": 0.5}),
    ("ht_64x64_hexagon", ("palr", 16), 16, ("imgl", 64, 64, 17), False, {"shape": "hexagon"}),
    ("ht_64x64_sharp1", ("palr", 16), 16, ("imgl", 64, 64, 18), False, {"sharpness": 1.0}),
    ("ht_64x64_sharp0.5", ("palr", 16), 16, ("imgl", 64, 64, 19), False, {"sharpness": 0.5}),
    ("ht_64x64_sharp4", ("palr", 16), 16, ("imgl", 64, 64, 20), False, {"sharpness": 4.0, "dot_gain": 1.3}),
    ("ht_48x48_p2", ("palr", 2, 11), 2, ("rnd", 48, 48, 21), False, {"cell_size": 4}),
    ("ht_64x64_p64", ("palr", 64), 64, ("rnd", 64, 64, 22), False, {"cell_size": 3}),
    ("ht_64x64_p256_g", ("palr", 256), 256, ("imgl", 64, 64, 23), True, {"cell_size": 2, "angle": 20.0}),
    ("ht_64x64_p1024", ("palr", 1024), 1024, ("rnd", 64, 64, 24), False, {"cell_size": 2}),
    ("ht_60x50_p1024_g", ("palr", 1024, 3), 1024, ("rnd", 60, 50, 25), True, {"cell_size": 3, "dot_gain": 2.5}),
    ("ht_dup_p17", ("dup", 12, 5), 17, ("rnd", 64, 64, 26), False, {"cell_size": 3}),
    ("ht_tie_grey10", ("grey10",), 26, ("tiegrey", 120, 160), False, {"angle": 0.0, "cell_size": 4}),
    ("ht_tie_grey10_rot", ("grey10",), 26, ("tiegrey", 120, 160), False, {"cell_size": 6}),
    ("ht_mediancut_16", ("none",), 16, ("imgl", 64, 80, 27), False, {}),
    ("ht_mediancut_64_g", ("none",), 64, ("imgl", 48, 72, 28), True, {"cell_size": 5}),
    ("ht_U27_grey", ("U", 27), 27, ("grey", 100, 130), False, {"angle": 60.0}),
    ("ht_121x203_p256", ("palr", 256), 256, ("rnd", 121, 203, 29), False, {"cell_size": 6, "dot_gain": 1.7}),
    ("ht_121x203_p16_g", ("palr", 16), 16, ("imgl", 121, 203, 30), True, {"angle": 75.0, "shape": "diamond"}),
    ("ht_1080x1920_p16", ("palr", 16), 16, ("imgl", 1080, 1920, 31), False, {}),
    ("ht_1080x1920_p256_dg1.5", ("palr", 256), 256, ("imgl", 1080, 1920, 32), False, {"dot_gain": 1.5, "sharpness": 4.0}),
    ("ht_2160x3840_p16", ("palr", 16), 16, ("imgl", 2160, 3840, 33), False, {}),
]

# HalftoneDitherStrategy(**params).dither(pixels f32, palette f32 (non-integer values), (h, w))
STRATEGY_CASES = [
    ("st_40x56_K5", 5, ("rnd", 40, 56, 40), {}),
    ("st_40x56_K40", 40, ("imgl", 40, 56, 41), {"cell_size": 5, "angle": 30.0, "dot_gain": 1.5}),
    ("st_33x47_K300", 300, ("rnd", 33, 47, 42), {"cell_size": 2, "shape": "square", "sharpness": 2.0}),
]

# _generate_halftone_screen_with_cells(h, w) of HalftoneDitherStrategy(**params)
SCREENS = [
    ("sc_23x31_default", 23, 31, {}),
    ("sc_23x31_cs7.5_a37.5", 23, 31, {"cell_size": 7.5, "angle": 37.5}),
    ("sc_17x40_a135_square", 17, 40, {"angle": 135.0, "shape": "square", "dot_gain": 0.5}),
    ("sc_40x17_am30_diamond", 40, 17, {"angle": -30.0, "shape": "diamond", "dot_gain": 2.0}),
    ("sc_32x32_a200_dg1.5", 32, 32, {"angle": 200.0, "dot_gain": 1.5, "min_dot_size": 0.1, "max_dot_size": 0.8}),
    ("sc_1x1", 1, 1, {}),
    ("sc_64x64_cs2_sharp4_dg3", 64, 64, {"cell_size": 2, "sharpness": 4.0, "dot_gain": 3.0}),
    ("sc_1080x1920_default", 1080, 1920, {}),
    ("sc_1080x1920_dg1.5_sharp4", 1080, 1920, {"dot_gain": 1.5, "sharpness": 4.0}),
]


def main():
    import PIL
    import scipy
    out = {"versions": {"numpy": np.__version__, "scipy": scipy.__version__, "pillow": PIL.__version__,
                        "python": sys.version.split()[0]},
           "cases": [], "strategy": [], "screens": []}
    npz = {}
    for name, pspec, ncol, ispec, gamma, params in CASES:
        t0 = time.time()
        arr = make_input(ispec)
        pal = make_palette(pspec)
        d = dl.ImageDitherer(ncol, dl.DitherMode.HALFTONE, None if pal is None else list(pal), gamma, dict(params))
        res = np.array(d.apply_dithering(Image.fromarray(arr)))
        used = [list(map(int, c)) for c in d.palette]
        case = {"name": name, "palette_spec": list(pspec), "num_colors": ncol, "input": list(ispec), "use_gamma": gamma,
                "params": params, "h": int(arr.shape[0]), "w": int(arr.shape[1]), "palette": used,
                "input_sha256": sha(arr), "output_sha256": sha(res)}
        if arr.shape[0] * arr.shape[1] <= 64 * 64 or arr.shape[0] == 1 or arr.shape[1] == 1:
            npz["out_" + name] = res
            case["full"] = True
        out["cases"].append(case)
        print(f"{name}: {time.time() - t0:.2f} s {case['output_sha256'][:16]}", flush=True)
    for name, K, ispec, params in STRATEGY_CASES:
        arr = make_input(ispec)
        h, w, _ = arr.shape
        pal = (np.random.RandomState(K).rand(K, 3) * 255.0).astype(np.float32)
        res = dl.HalftoneDitherStrategy(**params).dither(arr.reshape(-1, 3).astype(np.float32), pal, (h, w))
        npz["st_pal_" + name] = pal
        npz["st_out_" + name] = np.asarray(res)
        out["strategy"].append({"name": name, "K": K, "input": list(ispec), "params": params,
                                "output_sha256": sha(np.asarray(res))})
    for name, h, w, params in SCREENS:
        scr, cells = dl.HalftoneDitherStrategy(**params)._generate_halftone_screen_with_cells(h, w)
        scr, cells = np.asarray(scr), np.asarray(cells)
        ent = {"name": name, "h": h, "w": w, "params": params, "screen_dtype": str(scr.dtype),
               "cells_dtype": str(cells.dtype), "screen_sha256": sha(scr), "cells_sha256": sha(cells)}
        if h * w <= 64 * 64:
            npz["screen_" + name] = scr
            npz["cells_" + name] = cells
            ent["full"] = True
        out["screens"].append(ent)
    with open(os.path.join(HERE, "halftone.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    np.savez_compressed(os.path.join(HERE, "halftone.npz"), **npz)


if __name__ == "__main__":
    main()
