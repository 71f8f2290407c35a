"""CPU restatement of halftone dithering (HalftoneDitherStrategy.dither and _generate_halftone_screen_with_cells,
dithering_lib.py:1498-1695), written from its semantics -- test infrastructure only.

  * screen: (x_rot, y_rot) = (x cos - y sin, x sin + y cos) in float64 (cos, sin of np.radians(angle) from numpy); cell
    coordinates floor(r / cell_size), offset by their minimum, id = cy * max_x + cx (int32); the position inside the cell is
    numpy's floored remainder divided by cell_size, minus 0.5; distance by shape (an unknown one is a circle), normalised
    and clipped, raised to 1 / dot_gain (numpy's `**`: 0.5 is a square root, 2.0 a square, 1.0 the identity), mapped to
    [min_dot_size, max_dot_size], sharpened about 0.5 when sharpness != 1.0, clipped and rounded to float32
  * cell colour: exact channel sums / count of each cell in float64, nearest entry from the oracle's restated scipy
    KD-tree (oracle.oracle.Tree, k=1)
  * ink: float32 gray ((0.299 R + 0.587 G) + 0.114 B) / 255, darkness = 1 - gray; darkness > screen takes the cell's entry,
    otherwise the paper entry (first argmax of the palette's float32 brightness)
"""
import numpy as np

from oracle import oracle as orc

DEFAULTS = dict(cell_size=8, angle=45.0, dot_gain=1.0, min_dot_size=0.0, max_dot_size=1.0, shape="circle", sharpness=1.5)


def screen_with_cells(h, w, cell_size=8, angle=45.0, dot_gain=1.0, min_dot_size=0.0, max_dot_size=1.0, shape="circle",
                      sharpness=1.5):
    """(float32 [h, w] screen, int32 [h, w] cell ids) as the reference's _generate_halftone_screen_with_cells."""
    a = np.radians(angle)
    c, s = np.cos(a), np.sin(a)
    y, x = np.mgrid[0:h, 0:w]
    xr = x * c - y * s
    yr = x * s + y * c
    cx = np.floor(xr / cell_size).astype(np.int32)
    cy = np.floor(yr / cell_size).astype(np.int32)
    cx -= cx.min()
    cy -= cy.min()
    cells = cy * (cx.max() + 1) + cx
    dx = (xr % cell_size) / cell_size - 0.5
    dy = (yr % cell_size) / cell_size - 0.5
    if shape == "square":
        dist, max_dist = np.maximum(np.abs(dx), np.abs(dy)), 0.5
    elif shape == "diamond":
        dist, max_dist = np.abs(dx) + np.abs(dy), 1.0
    else:
        dist, max_dist = np.sqrt(dx ** 2 + dy ** 2), 0.5
    t = np.clip(dist / max_dist, 0.0, 1.0) ** (1.0 / dot_gain)
    t = min_dot_size + t * (max_dot_size - min_dot_size)
    if sharpness != 1.0:
        t = 0.5 + (t - 0.5) * sharpness
    return np.clip(t, 0.0, 1.0).astype(np.float32), cells


def paper_index(pal_f32):
    pal = np.asarray(pal_f32, np.float32)
    return int(np.argmax(0.299 * pal[:, 0] + 0.587 * pal[:, 1] + 0.114 * pal[:, 2]))


def halftone_idx(px_f32, pal_f32, **params):
    """float32 pixels [h, w, 3] (the values the strategy sees) -> int palette indices [h, w]."""
    h, w, _ = px_f32.shape
    p = dict(DEFAULTS, **params)
    screen, cells = screen_with_cells(h, w, **p)
    pal = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    ids = cells.ravel()
    flat = px_f32.reshape(-1, 3).astype(np.float64)
    n = int(ids.max()) + 1
    cnt = np.bincount(ids, minlength=n)
    sums = np.stack([np.bincount(ids, weights=flat[:, k], minlength=n) for k in range(3)], 1)
    used = np.nonzero(cnt)[0]
    _, ii = orc.Tree(pal).query(sums[used] / cnt[used, None], 1)
    cell_idx = np.zeros(n, np.int64)
    cell_idx[used] = ii[:, 0]
    gray = (np.float32(0.299) * px_f32[..., 0] + np.float32(0.587) * px_f32[..., 1]) + np.float32(0.114) * px_f32[..., 2]
    dark = np.float32(1.0) - gray / np.float32(255.0)
    return np.where(dark > screen, cell_idx[cells], paper_index(pal))


def halftone_u8(arr, pal_f32, out_colors, lut_in=None, **params):
    """uint8 [h, w, 3] -> uint8 [h, w, 3] (ImageDitherer.apply_dithering's view: lut_in first, out_colors last)."""
    h, w, _ = arr.shape
    if h == 0 or w == 0:
        return np.zeros_like(arr)
    src = np.asarray(lut_in)[arr] if lut_in is not None else arr
    return np.asarray(out_colors, np.uint8)[halftone_idx(src.astype(np.float32), pal_f32, **params)]


def apply(arr, palette, use_gamma=False, **params):
    """ImageDitherer(..., DitherMode.HALFTONE, palette, use_gamma, params).apply_dithering on a uint8 array."""
    pal_f32, out_colors, lut_in = orc.prepare_palette(palette, use_gamma)
    return halftone_u8(arr, pal_f32, out_colors, lut_in, **params)
