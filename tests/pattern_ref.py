"""Pattern (Knoll) dithering as include/ditherpie_hip_pattern.h defines it, in numpy: the plain statement the GPU kernel is
held to.  All integer arithmetic.  nearest() is the CPU oracle's nearest-only search (oracle.ordered_u8(..., None, "none",
want_idx=True)): scipy's KD-tree order on ties, no lut_in -- the n queries of every pixel are evaluated as one image per
iteration, which is a valid uint8 image because of the clamp."""
import numpy as np


def bayer_rank(m):
    """B_2 = [[0, 2], [3, 1]], B_2m = [[4B, 4B + 2], [4B + 3, 4B + 1]]: a permutation of 0 .. m*m - 1."""
    if m not in (2, 4, 8):
        raise ValueError(m)
    b = np.array([[0, 2], [3, 1]], np.int64)
    while b.shape[0] < m:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


def palette_ints(pal_f32):
    """C[k] = trunc(pal_f32[k]) and L[k] = 299 r + 587 g + 114 b."""
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3)
    assert pal.min() >= 0 and pal.max() <= 255
    c = np.trunc(pal).astype(np.int64)
    return c, 299 * c[:, 0] + 587 * c[:, 1] + 114 * c[:, 2]


def pattern_indices(orc, img, pal_f32, out_colors, lut_in, m, strength256, y0=0, x0=0):
    """img [H,W,3] uint8 -> the chosen palette index per pixel [H,W] (int64)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, _ = img.shape
    pal_f32 = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    assert 0 <= strength256 <= 256 and 1 <= pal_f32.shape[0] <= 256
    n = m * m
    C, L = palette_ints(pal_f32)
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64)
    e = np.zeros_like(c)
    ks = np.empty((n, h, w), np.int64)
    for i in range(n):
        t = np.clip(c + ((e * strength256) >> 8), 0, 255).astype(np.uint8)       # >> on int64 floors
        ks[i] = orc.ordered_u8(t, pal_f32, out_colors, None, "none", want_idx=True)[1]
        e += c - C[ks[i]]
    key = L[ks] * 256 + ks                                                      # ascending by (L[k], k); k < 256
    k_sorted = np.take_along_axis(ks, np.argsort(key, axis=0, kind="stable"), axis=0)
    B = bayer_rank(m)
    yy = (y0 + np.arange(h)) % m
    xx = (x0 + np.arange(w)) % m
    pick = B[yy[:, None], xx[None, :]]
    return np.take_along_axis(k_sorted, pick[None], axis=0)[0]


def pattern_u8(orc, img, pal_f32, out_colors, lut_in, m, strength256, y0=0, x0=0):
    """img [H,W,3] uint8 -> the dithered image [H,W,3] uint8."""
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    return out_colors[pattern_indices(orc, img, pal_f32, out_colors, lut_in, m, strength256, y0, x0)]


def pattern_frames(orc, frames, pal_f32, out_colors, lut_in, m, strength256, y0=0, x0=0):
    return np.stack([pattern_u8(orc, f, pal_f32, out_colors, lut_in, m, strength256, y0, x0) for f in frames])
