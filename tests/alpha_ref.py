"""Transparency as include/ditherpie_hip_alpha.h defines it, in numpy / Python: the plain statements the kernels and the host entry
points are held to.  All integer arithmetic.  mask / matte / split / key / join are array expressions; idiff_masked_indices and
dotdiff_masked_indices are the PUSH-form loops of tests/idiff_ref.py and tests/dotdiff_ref.py with the mask rules written in: a
masked pixel is skipped (its output is `fill`), a contribution sent to a masked pixel is lost (integer diffusion) or is not sent at
all because the masked neighbour is not in E (dot diffusion).  nearest() is what the `orc` adapter answers for a nearest-only search
(oracle.ordered_u8(..., None, "none", want_idx=True)), memoised on the query."""
import numpy as np

import dotdiff_ref as dr
import idiff_ref as ir
from pattern_ref import bayer_rank

MODES = ("threshold", "ordered")
MATRICES = (2, 4, 8)


def mask_of(alpha, mode="threshold", threshold=128, m=4, y0=0, x0=0):
    """alpha [..., H, W] uint8 -> mask uint8 of the same shape: 1 transparent, 0 opaque."""
    a = np.asarray(alpha).astype(np.int64)
    if mode == "threshold":
        assert 0 <= threshold <= 256
        return (a < threshold).astype(np.uint8)
    assert mode == "ordered" and m in MATRICES
    h, w = a.shape[-2:]
    B = bayer_rank(m)[((y0 + np.arange(h)) % m)[:, None], ((x0 + np.arange(w)) % m)[None, :]]
    return (2 * m * m * a < 255 * (2 * B + 1)).astype(np.uint8)


def opaque_per_tile(a, m):
    """How many pixels of a full m x m tile of constant alpha a are opaque."""
    return (2 * m * m * a + 255) // 510


def matte_of(rgba, matte=None):
    """rgba [..., 4] uint8 -> the RGB handed to the ditherer [..., 3] uint8."""
    rgba = np.asarray(rgba, np.uint8)
    if matte is None:
        return np.ascontiguousarray(rgba[..., :3])
    c, a = rgba[..., :3].astype(np.int64), rgba[..., 3:4].astype(np.int64)
    return ((c * a + np.asarray(matte, np.int64) * (255 - a) + 127) // 255).astype(np.uint8)


def split(rgba, mode="threshold", threshold=128, m=4, matte=None, y0=0, x0=0):
    """rgba [N,H,W,4] -> (rgb [N,H,W,3], mask [N,H,W], masked [N] int64)."""
    rgba = np.asarray(rgba, np.uint8)
    mask = mask_of(rgba[..., 3], mode, threshold, m, y0, x0)
    return matte_of(rgba, matte), mask, mask.sum(axis=(-2, -1), dtype=np.int64)


def key(planes, mask, k):
    return np.where(np.asarray(mask) != 0, np.uint8(k), np.asarray(planes, np.uint8)).astype(np.uint8)


def join(rgb, mask, fill=(0, 0, 0)):
    rgb, hidden = np.asarray(rgb, np.uint8), np.asarray(mask) != 0
    out = np.empty(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.where(hidden[..., None], np.asarray(fill, np.uint8), rgb)
    out[..., 3] = np.where(hidden, 0, 255)
    return out


def _nearest(orc, memo, t, pal_f32, out_colors):
    k = memo.get(t)
    if k is None:
        k = memo[t] = int(orc.ordered_u8(np.array(t, np.uint8).reshape(1, 1, 3), pal_f32, out_colors, None, "none", want_idx=True)[1].reshape(-1)[0])
    return k


def idiff_masked_indices(orc, img, mask, pal_f32, out_colors, lut_in, taps, divisor, strength256):
    """img [H,W,3] uint8, mask [H,W] -> the chosen palette index per pixel [H,W] (int64), -1 at the masked pixels."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, _ = img.shape
    hidden = (np.asarray(mask).reshape(h, w) != 0).tolist()
    pal_f32 = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    taps = ir.check_taps(taps, divisor, strength256)
    q = ir.shares(taps, divisor, strength256)
    C = np.trunc(pal_f32).astype(np.int64).tolist()
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64).tolist()
    acc = [[[0, 0, 0] for _ in range(w)] for _ in range(h)]
    idx = np.full((h, w), -1, np.int64)
    memo = {}
    for y in range(h):
        for x in range(w):
            if hidden[y][x]:
                continue                                              # out = fill; acc is never read, no error, no contributions
            a = acc[y][x]
            u = [min(max(16 * c[y][x][ch] + a[ch], 0), 4080) for ch in range(3)]
            k = _nearest(orc, memo, ((u[0] + 8) >> 4, (u[1] + 8) >> 4, (u[2] + 8) >> 4), pal_f32, out_colors)
            idx[y, x] = k
            e = [u[ch] - 16 * C[k][ch] for ch in range(3)]
            for (dx, dy, _), qk in zip(taps, q):
                ny, nx = y + dy, x + dx
                if ny < h and 0 <= nx < w:                            # (a contribution to a masked pixel lands in an acc nobody reads)
                    d = acc[ny][nx]
                    for ch in range(3):
                        s = (abs(e[ch]) * qk) >> 16
                        d[ch] += s if e[ch] >= 0 else -s
    return idx


def dotdiff_masked_indices(orc, img, mask, pal_f32, out_colors, lut_in, classes, strength256):
    """img [H,W,3] uint8, mask [H,W] -> the chosen palette index per pixel [H,W] (int64), -1 at the masked pixels."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, _ = img.shape
    hidden = (np.asarray(mask).reshape(h, w) != 0).tolist()
    pal_f32 = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    assert 0 <= strength256 <= 256
    M = dr.check_matrix(classes)
    m = M.shape[0]
    C = np.trunc(pal_f32).astype(np.int64).tolist()
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64).tolist()
    cls = M[(np.arange(h) % m)[:, None], (np.arange(w) % m)[None, :]].tolist()
    acc = [[[0, 0, 0] for _ in range(w)] for _ in range(h)]
    idx = np.full((h, w), -1, np.int64)
    memo = {}
    order = sorted((cls[y][x], y, x) for y in range(h) for x in range(w))
    for k_cls, y, x in order:
        if hidden[y][x]:
            continue                                                  # out = fill; it hands on nothing
        a = acc[y][x]
        u = [min(max(16 * c[y][x][ch] + a[ch], 0), 4080) for ch in range(3)]
        k = _nearest(orc, memo, ((u[0] + 8) >> 4, (u[1] + 8) >> 4, (u[2] + 8) >> 4), pal_f32, out_colors)
        idx[y, x] = k
        e = [u[ch] - 16 * C[k][ch] for ch in range(3)]
        E = [(y + dy, x + dx, wt) for dy, dx, wt in dr.NEIGHBOURS
             if 0 <= y + dy < h and 0 <= x + dx < w and cls[y + dy][x + dx] > k_cls and not hidden[y + dy][x + dx]]
        W = sum(wt for _, _, wt in E)
        for ny, nx, wt in E:
            d = acc[ny][nx]
            for ch in range(3):
                num = e[ch] * wt * strength256
                s = abs(num) // (256 * W)                             # trunc toward zero, C's '/'
                d[ch] += s if num >= 0 else -s
    return idx


def colours(idx, out_colors, fill):
    """Indices with -1 at the masked pixels -> the bytes the kernels write."""
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    return np.where((idx < 0)[..., None], np.asarray(fill, np.uint8), out_colors[np.maximum(idx, 0)]).astype(np.uint8)


def idiff_masked_u8(orc, img, mask, pal_f32, out_colors, lut_in, taps, divisor, strength256, fill=(0, 0, 0)):
    return colours(idiff_masked_indices(orc, img, mask, pal_f32, out_colors, lut_in, taps, divisor, strength256), out_colors, fill)


def dotdiff_masked_u8(orc, img, mask, pal_f32, out_colors, lut_in, classes, strength256, fill=(0, 0, 0)):
    return colours(dotdiff_masked_indices(orc, img, mask, pal_f32, out_colors, lut_in, classes, strength256), out_colors, fill)


MASKS = ("half", "sixteenth", "opaque", "transparent", "one_opaque", "checker", "first_col", "last_col", "first_row", "rows_62_65")


def mask_family(name, h, w, seed=0):
    """The masks of the suite: [H,W] uint8 whose transparent pixels carry 1 -- or, for the random ones, any non-zero byte."""
    rng = np.random.default_rng(seed)
    k = np.zeros((h, w), np.uint8)
    if name == "half":
        k = (rng.integers(0, 2, (h, w)) * rng.integers(1, 256, (h, w))).astype(np.uint8)
    elif name == "sixteenth":
        k = ((rng.integers(0, 16, (h, w)) == 0) * rng.integers(1, 256, (h, w))).astype(np.uint8)
    elif name == "transparent":
        k[:] = 1
    elif name == "one_opaque":
        k[:] = 1
        k[h // 2, w // 2] = 0
    elif name == "checker":
        k = ((np.add.outer(np.arange(h), np.arange(w)) & 1)).astype(np.uint8)
    elif name == "first_col":
        k[:, 0] = 1
    elif name == "last_col":
        k[:, -1] = 1
    elif name == "first_row":
        k[0, :] = 1
    elif name == "rows_62_65":
        k[62:66, :] = 1
    elif name != "opaque":
        raise ValueError(name)
    return np.ascontiguousarray(k)
