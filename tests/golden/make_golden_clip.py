#!/usr/bin/env python3
"""Record the REFERENCE's median-cut palettes of small clips (build container only): tests/golden/clip.{json,npz}.

Run:  python tests/golden/make_golden_clip.py        (needs the reference checkout, as make_golden.py does; seconds)

For each clip the taken frames are stacked top to bottom into one image -- linearised through the reference's own uint8
gamma table first under use_gamma, as ImageDitherer.apply_dithering does before it cuts -- and the reference's
ColorReducer.reduce_colors(image, n) is recorded for several n.  Frames come from the seeded formulas of oracle/oracle.py, so
the tests regenerate them; only DATA is stored: clip.json (the clip specifications and the palettes) and clip.npz (the
stacked images' distinct colours in order of first occurrence, for the CPU tier's host-tail check)."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DITHER_PIE_REFERENCE", "/root/reference")

sys.modules.setdefault("pywt", types.ModuleType("pywt"))
sys.path.insert(0, REF)
import dithering_lib as dl  # noqa: E402  (the reference)
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from clip_palette_ref import distinct_first  # noqa: E402
from clip_spec import clip_frames  # noqa: E402

NUM_COLORS = [2, 16, 20, 64, 256]

# name -> (frame specifications, use_gamma); a frame is ["rnd", h, w, seed] | ["imgl", h, w, seed, kind] | ["grad", h, w] |
# ["flat", h, w, [r, g, b]] | ["few", h, w, n_colours, seed] | ["sub", h, w, of_frame, seed] (pixels drawn from an earlier frame)
CLIPS = {
    "rnd_2x16x24": ([["rnd", 16, 24, 1], ["rnd", 16, 24, 2]], False),
    "rnd_5x16x24": ([["rnd", 16, 24, 10 + i] for i in range(5)], False),
    "imgl_3x64x48": ([["imgl", 64, 48, 3, "smooth"], ["imgl", 64, 48, 4, "dark"], ["grad", 64, 48]], False),
    "mixed_geometry": ([["rnd", 16, 24, 5], ["imgl", 48, 64, 6, "smooth"], ["grad", 33, 17]], False),
    "later_frames_add_nothing": ([["rnd", 32, 40, 7], ["sub", 32, 40, 0, 8], ["sub", 24, 16, 0, 9]], False),
    "first_frame_flat_black": ([["flat", 48, 64, [0, 0, 0]], ["imgl", 48, 64, 11, "smooth"], ["rnd", 48, 64, 12]], False),
    "few_colours": ([["few", 32, 32, 8, 13], ["few", 32, 32, 8, 13], ["flat", 32, 32, [9, 9, 9]]], False),
    "gamma_4x32x48": ([["imgl", 32, 48, 14, "smooth"], ["rnd", 32, 48, 15], ["grad", 32, 48], ["imgl", 32, 48, 16, "dark"]], True),
}


def main():
    cases, arrays = {}, {}
    for name, (specs, gamma) in CLIPS.items():
        frames = clip_frames(specs)
        stack = np.concatenate([f.reshape(-1, 3) for f in frames]).reshape(-1, 1, 3)   # one pixel wide: getdata() order is stream order
        if gamma:   # the reference's own linearisation (ImageDitherer.apply_dithering under use_gamma)
            stack = np.clip(dl.DitherUtils.srgb_to_linear(stack.astype(np.float32) / 255.0) * 255.0, 0, 255).astype(np.uint8)
        img = Image.fromarray(np.ascontiguousarray(stack), "RGB")
        pals = {str(n): [list(map(int, c)) for c in dl.ColorReducer.reduce_colors(img, n)] for n in NUM_COLORS}
        cases[name] = {"frames": specs, "use_gamma": gamma, "palettes": pals, "n_pixels": int(stack.shape[0])}
        arrays[name + "/distinct"] = distinct_first(stack)
    with open(os.path.join(HERE, "clip.json"), "w") as f:
        json.dump({"num_colors": NUM_COLORS, "clips": cases}, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "clip.npz"), **arrays)
    print({k: (v["n_pixels"], len(arrays[k + "/distinct"])) for k, v in cases.items()})


if __name__ == "__main__":
    main()
