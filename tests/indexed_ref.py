"""The contract of the indexed output (include/ditherpie_hip_indexed.h), stated in numpy.

For K output colours C[0..K) (uint8 RGB, duplicates allowed) and an RGB pixel p: index(p) is the LOWEST j with
C[j] == p; a pixel equal to no entry is missing: index 0, counted; decode(index(p)) == p for every other pixel."""
import numpy as np


def _codes(rgb):
    a = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64)
    return a[:, 0] | (a[:, 1] << 8) | (a[:, 2] << 16)


def lowest_index(colors):
    """-> int64 [K]: for every entry of `colors` the lowest position holding the same colour."""
    code = _codes(colors)
    first = {}
    for j, c in enumerate(code.tolist()):
        first.setdefault(c, j)
    return np.array([first[c] for c in code.tolist()], np.int64)


def to_indices(rgb, colors):
    """rgb [...,3] uint8 -> (index [...] int64, missing [...] bool, number of missing pixels)."""
    rgb = np.asarray(rgb, np.uint8)
    uniq, first = np.unique(_codes(colors), return_index=True)           # first: the lowest position of every distinct colour
    px = _codes(rgb)
    pos = np.minimum(np.searchsorted(uniq, px), len(uniq) - 1)
    idx = np.where(uniq[pos] == px, first[pos], -1).reshape(rgb.shape[:-1]).astype(np.int64)
    missing = idx < 0
    return np.where(missing, 0, idx), missing, int(missing.sum())


def from_indices(index, colors):
    """index [...] (any integer type; int16 planes are read as unsigned) -> (rgb [...,3] uint8, bad [...] bool, number of
    bad indices): an index >= K decodes to entry 0 and is counted."""
    index = np.asarray(index)
    if index.dtype == np.int16:
        index = index.view(np.uint16)
    i = index.astype(np.int64)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    bad = (i < 0) | (i >= len(colors))
    return colors[np.where(bad, 0, i)], bad, int(bad.sum())


def nearest_coords(n_in, n_out):
    """Source positions of Pillow's NEAREST resize (ImagingScaleAffine): xo accumulated in double from 0.5 * scale."""
    a = float(n_in) / float(n_out)
    xo = a * 0.5
    out = np.empty(n_out, np.int64)
    for x in range(n_out):
        out[x] = min(int(xo), n_in - 1)
        xo = xo + a
    return out


def resize_nearest_plane(planes, oh, ow):
    """planes [N,H,W] -> [N,oh,ow] by numpy indexing with Pillow's coordinates."""
    planes = np.asarray(planes)
    ys, xs = nearest_coords(planes.shape[1], oh), nearest_coords(planes.shape[2], ow)
    return planes[:, ys][:, :, xs]
