"""CPU restatement of Riemersma dithering (RiemersmaDitherStrategy.dither, dithering_lib.py:812-841), written from its
semantics -- test infrastructure only.

  * path: index t of the dim x dim square (dim = the next power of two of max(h, w)) is (row, col) = (y, x), with (x, y)
    from the reference's hilbert_xy level loop; only indices with row < h and col < w are visited
  * pull form: at in-image step p the value starts as the input (float32 of the byte, through lut_in under use_gamma) and
    receives, from the in-image steps at p-4, p-3, p-2, p-1 in that order, fl32(e * w) with w = 3/16, 5/16, 1/16, 7/16,
    one float32 add and a clip to [0, 255] after each
  * nearest entry: the oracle's restated scipy KD-tree (oracle.oracle.Tree, k=1), so no scipy is needed
  * error e = v - pal_f32[idx] in float32; output = out_colors[idx]
A per-step Python loop: fine up to ~300 x 300 pixels.
"""
from collections import deque

import numpy as np

from oracle import oracle as orc

_W = {1: np.float32(7 / 16), 2: np.float32(1 / 16), 3: np.float32(5 / 16), 4: np.float32(3 / 16)}


def path_rc(dim):
    """(row, col) int64 arrays of every path index of the dim x dim Hilbert curve."""
    bits = dim.bit_length() - 1
    t = np.arange(dim * dim, dtype=np.int64)
    x = np.zeros_like(t)
    y = np.zeros_like(t)
    for lvl in range(bits):
        s = 1 << lvl
        rx = (t >> 1) & 1
        ry = (t ^ rx) & 1
        refl = (ry == 0) & (rx == 1)
        x = np.where(refl, s - 1 - x, x)
        y = np.where(refl, s - 1 - y, y)
        swap = ry == 0
        x, y = np.where(swap, y, x), np.where(swap, x, y)
        x = x + s * rx
        y = y + s * ry
        t = t >> 2
    return y, x


def riemersma_u8(arr, pal_f32, out_colors, lut_in=None):
    """uint8 [h, w, 3] -> uint8 [h, w, 3]; pal_f32 [K, 3] float32 as the KD-tree sees it, out_colors [K, 3] uint8."""
    h, w, _ = arr.shape
    out = np.zeros_like(arr)
    if h == 0 or w == 0:
        return out
    dim = 1
    while dim < max(h, w):
        dim *= 2
    rows, cols = path_rc(dim)
    inside = (rows < h) & (cols < w)
    steps = np.nonzero(inside)[0]
    rows, cols = rows[inside], cols[inside]
    src = arr[rows, cols]
    if lut_in is not None:
        src = np.asarray(lut_in)[src]
    src = src.astype(np.float32)
    pal = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    tree = orc.Tree(pal)
    hist = deque(maxlen=4)   # (path index, error) of the last four in-image steps, oldest first
    lo, hi = np.float32(0), np.float32(255)
    for k in range(len(steps)):
        p = int(steps[k])
        v = src[k].copy()
        for q, e in hist:
            d = p - q
            if 1 <= d <= 4:
                v = np.minimum(np.maximum(v + e * _W[d], lo), hi)
        _, ii = tree.query(v, 1)
        j = int(ii[0, 0])
        hist.append((p, v - pal[j]))
        out[rows[k], cols[k]] = out_colors[j]
    return out


def apply(arr, palette, use_gamma=False):
    """ImageDitherer(..., DitherMode.RIEMERSMA, palette, use_gamma).apply_dithering on a uint8 array (explicit palette)."""
    pal_f32, out_colors, lut_in = orc.prepare_palette(palette, use_gamma)
    return riemersma_u8(arr, pal_f32, out_colors, lut_in)
