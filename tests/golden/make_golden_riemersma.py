#!/usr/bin/env python3
"""Record the Riemersma (Hilbert-curve error diffusion) fixtures from the REFERENCE itself (build container only).

Run:  python tests/golden/make_golden_riemersma.py      (needs the reference checkout; ~5 minutes)

Imports dobrosketchkun/dither_pie's dithering_lib the way make_golden.py does (an in-memory stub stands in for the unused
`pywt` import; DITHER_PIE_REFERENCE names the checkout) and records, for seeded synthetic inputs and palettes (formulas
in oracle/oracle.py: rnd / grad / palr / generate_uniform_palette), the outputs of
ImageDitherer(..., DitherMode.RIEMERSMA, ...).apply_dithering.  Only DATA is stored:
  riemersma.json  the cases (input / palette specs, use_gamma), the palettes used, the sha256 of every output, versions
  riemersma.npz   _hilbert_order(n) for n = 1, 2, 4, ..., 64, _next_power_of_two(x) for x = 0 .. 1100, and the full
                  outputs of the cases of at most 64 x 64 pixels
"""
import hashlib
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DITHER_PIE_REFERENCE", "/root/reference")

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
    raise ValueError(spec)


# (name, palette spec, num_colors, input spec, use_gamma)
CASES = [
    ("rm_1x1_p2", ("palr", 2), 2, ("rnd", 1, 1, 1), False),
    ("rm_1x300_p8", ("palr", 8), 8, ("rnd", 1, 300, 2), False),
    ("rm_300x1_p16_g", ("palr", 16), 16, ("rnd", 300, 1, 3), True),
    ("rm_37x53_p2", ("palr", 2, 11), 2, ("rnd", 37, 53, 4), False),
    ("rm_37x53_p17", ("palr", 17), 17, ("rnd", 37, 53, 4), False),
    ("rm_37x53_p17_g", ("palr", 17), 17, ("rnd", 37, 53, 4), True),
    ("rm_64x64_p64", ("palr", 64), 64, ("rnd", 64, 64, 5), False),
    ("rm_64x64_p65_g", ("palr", 65), 65, ("rnd", 64, 64, 5), True),
    ("rm_64x64_p256", ("palr", 256), 256, ("grad", 64, 64), False),
    ("rm_37x53_p257_g", ("palr", 257), 257, ("rnd", 37, 53, 6), True),
    ("rm_64x64_p1024", ("palr", 1024), 1024, ("rnd", 64, 64, 7), False),
    ("rm_37x53_p1024_g", ("palr", 1024, 3), 1024, ("rnd", 37, 53, 8), True),
    ("rm_120x200_p256", ("palr", 256), 256, ("rnd", 120, 200, 9), False),
    ("rm_120x200_p257_g", ("palr", 257), 257, ("imgl", 120, 200, 10), True),
    ("rm_120x200_U16", ("U", 16), 16, ("grad", 120, 200), False),
    ("rm_grey_U8", ("U", 8), 8, ("grey", 64, 256), False),
    ("rm_grey_U27", ("U", 27), 27, ("grey", 100, 130), False),
    ("rm_grey_U64_g", ("U", 64), 64, ("grey", 64, 256), True),
    ("rm_dup_p17", ("dup", 12, 5), 17, ("rnd", 64, 64, 12), False),
    ("rm_mediancut_16", ("none",), 16, ("imgl", 64, 80, 13), False),
    ("rm_mediancut_64_g", ("none",), 64, ("imgl", 48, 72, 14), True),
    ("rm_540x960_p64", ("palr", 64), 64, ("imgl", 540, 960, 15), False),
    ("rm_1080x1920_p16", ("palr", 16), 16, ("imgl", 1080, 1920, 16), False),
]


def main():
    import PIL
    import scipy
    out = {"versions": {"numpy": np.__version__, "scipy": scipy.__version__, "pillow": PIL.__version__,
                        "python": sys.version.split()[0]},
           "cases": [], "hilbert": {}, "next_power_of_two": {}}
    npz = {}
    for k in range(7):
        n = 1 << k
        o = dl._hilbert_order(n)
        npz[f"hilbert_{n}"] = o.astype(np.int32)
        out["hilbert"][str(n)] = sha(o.astype(np.int32))
    xs = np.arange(0, 1101)
    npz["npot_x"] = xs.astype(np.int64)
    npz["npot"] = np.array([dl._next_power_of_two(int(x)) for x in xs], np.int64)
    for name, pspec, ncol, ispec, gamma in CASES:
        t0 = time.time()
        arr = make_input(ispec)
        pal = make_palette(pspec)
        d = dl.ImageDitherer(ncol, dl.DitherMode.RIEMERSMA, None if pal is None else list(pal), gamma, {})
        res = np.array(d.apply_dithering(Image.fromarray(arr)))
        used = [list(map(int, c)) for c in d.palette]
        case = {"name": name, "palette_spec": list(pspec), "num_colors": ncol, "input": list(ispec), "use_gamma": gamma,
                "h": int(arr.shape[0]), "w": int(arr.shape[1]), "palette": used, "input_sha256": sha(arr),
                "output_sha256": sha(res)}
        if arr.shape[0] * arr.shape[1] <= 64 * 64 or name.startswith("rm_1x") or name.startswith("rm_300x"):
            npz["out_" + name] = res
            case["full"] = True
        out["cases"].append(case)
        print(f"{name}: {time.time() - t0:.1f} s {case['output_sha256'][:16]}", flush=True)
    with open(os.path.join(HERE, "riemersma.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    np.savez_compressed(os.path.join(HERE, "riemersma.npz"), **npz)


if __name__ == "__main__":
    main()
