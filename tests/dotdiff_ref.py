"""Dot diffusion as include/ditherpie_hip_dotdiff.h defines it, in numpy: the plain statement the GPU kernel is held to.  All
integer arithmetic.  It goes class by class (all pixels of a class at once: they are never neighbours of one another in a
way that matters, a pixel only hands on to HIGHER classes), so it knows nothing of the level schedule the kernel walks.
nearest() is the CPU oracle's nearest-only search (oracle.ordered_u8(..., None, "none", want_idx=True)): scipy's KD-tree order
on ties, no lut_in.  reach() and levels() are the longest-increasing-path definitions, by relaxation."""
import numpy as np

KNUTH = np.array([
    [34, 48, 40, 32, 29, 15, 23, 31],
    [42, 58, 56, 53, 21, 5, 7, 10],
    [50, 62, 61, 45, 13, 1, 2, 18],
    [38, 46, 54, 37, 25, 17, 9, 26],
    [28, 14, 22, 30, 35, 49, 41, 33],
    [20, 4, 6, 11, 43, 59, 57, 52],
    [12, 0, 3, 19, 51, 63, 60, 44],
    [24, 16, 8, 27, 39, 47, 55, 36]], np.int64)

NEIGHBOURS = [(dy, dx, 2 if dy == 0 or dx == 0 else 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]
MAX_REACH = 16


def check_matrix(classes):
    m = np.asarray(classes)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] not in (2, 4, 8, 16):
        raise ValueError(f"class matrix must be m x m with m in (2, 4, 8, 16), not {m.shape}")
    if sorted(m.reshape(-1).tolist()) != list(range(m.size)):
        raise ValueError("class matrix is not a permutation")
    return m.astype(np.int64)


def levels(classes):
    """level[cell] = the longest path of king moves through the tiled matrix that ends in the cell with strictly increasing
    classes.  Bellman-Ford style: relax until nothing changes (at most m*m rounds: classes increase along a path)."""
    M = check_matrix(classes)
    lv = np.zeros_like(M)
    for _ in range(M.size + 1):
        new = lv.copy()
        for dy, dx, _w in NEIGHBOURS:
            nb_cls, nb_lv = np.roll(M, (dy, dx), (0, 1)), np.roll(lv, (dy, dx), (0, 1))
            new = np.maximum(new, np.where(nb_cls < M, nb_lv + 1, 0))
        if np.array_equal(new, lv):
            return lv
        lv = new
    raise AssertionError("no fixed point")


def reach(classes):
    return int(levels(classes).max())


def palette_ints(pal_f32):
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3)
    assert pal.min() >= 0 and pal.max() <= 255
    return np.trunc(pal).astype(np.int64)


def dotdiff_indices(orc, img, pal_f32, out_colors, lut_in, classes, strength256, want_acc=False):
    """img [H,W,3] uint8 -> the chosen palette index per pixel [H,W] (int64) (and the largest |acc| seen)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, _ = img.shape
    pal_f32 = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    assert 0 <= strength256 <= 256 and 1 <= pal_f32.shape[0] <= 256
    M = check_matrix(classes)
    m = M.shape[0]
    C = palette_ints(pal_f32)
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64)
    cls = M[(np.arange(h) % m)[:, None], (np.arange(w) % m)[None, :]]
    # W per pixel: the weights of the neighbours inside the image whose class is greater
    W = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for dy, dx, wt in NEIGHBOURS:
        ny, nx = yy + dy, xx + dx
        ok = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        W[ok] += wt * (cls[ny[ok], nx[ok]] > cls[ok])
    acc = np.zeros((h, w, 3), np.int64)
    idx = np.zeros((h, w), np.int64)
    big = 0
    for k in range(m * m):
        py, px = np.nonzero(cls == k)
        if not len(py):
            continue
        big = max(big, int(np.abs(acc[py, px]).max()))
        u = np.clip(16 * c[py, px] + acc[py, px], 0, 4080)
        t = ((u + 8) >> 4).astype(np.uint8)
        ks = orc.ordered_u8(t.reshape(1, -1, 3), pal_f32, out_colors, None, "none", want_idx=True)[1].reshape(-1)
        idx[py, px] = ks
        e = u - 16 * C[ks]
        for dy, dx, wt in NEIGHBOURS:
            ny, nx = py + dy, px + dx
            ok = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
            ok[ok] &= cls[ny[ok], nx[ok]] > k
            if not ok.any():
                continue
            num = e[ok] * (wt * strength256)
            den = 256 * W[py[ok], px[ok]][:, None]
            share = np.sign(num) * (np.abs(num) // den)                 # trunc toward zero, C's '/'
            np.add.at(acc, (ny[ok], nx[ok]), share)
    return (idx, big) if want_acc else idx


def dotdiff_u8(orc, img, pal_f32, out_colors, lut_in, classes, strength256):
    """img [H,W,3] uint8 -> the dithered image [H,W,3] uint8."""
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    return out_colors[dotdiff_indices(orc, img, pal_f32, out_colors, lut_in, classes, strength256)]


def dotdiff_frames(orc, frames, pal_f32, out_colors, lut_in, classes, strength256):
    return np.stack([dotdiff_u8(orc, f, pal_f32, out_colors, lut_in, classes, strength256) for f in frames])
