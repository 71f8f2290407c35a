"""Cell-palette dithering as include/ditherpie_hip_cells.h defines it, in numpy: the plain statement the GPU kernel is held to.
All integer arithmetic; brute force over itertools.combinations, np.argmin (the first of equal values) for both tie rules."""
import itertools

import numpy as np

from pattern_ref import bayer_rank

CELL_SIZES = (4, 8, 16)
MATRICES = (2, 4, 8)


def mask_of(indices):
    m = 0
    for j in indices:
        m |= 1 << int(j)
    return m


def bits_of(mask):
    return [j for j in range(16) if (mask >> j) & 1]


def candidates(K, k, fixed, groups):
    """The masks S = T | fixed in the order of the definition: group by group, within a group the k-subsets of the group's
    entries outside `fixed` in lexicographic order of their ascending index tuples.  ValueError where the definition has no
    candidates: K outside 1 .. 16, k outside 1 .. 4, no or more than 4 groups, a bit at or above K, an empty group, a
    group with fewer than k entries outside fixed."""
    groups = list(groups)
    if not (1 <= K <= 16 and 1 <= k <= 4 and 1 <= len(groups) <= 4) or fixed >> K:
        raise ValueError((K, k, fixed, groups))
    out = []
    for g in groups:
        if g == 0 or g >> K:
            raise ValueError((K, g))
        free = [j for j in bits_of(g) if not (fixed >> j) & 1]
        if len(free) < k:
            raise ValueError((g, fixed, k))
        out.extend(mask_of(t) | fixed for t in itertools.combinations(free, k))   # combinations of a sorted list: lexicographic
    return out


def perturbation(h, w, m, spread):
    """floor(((2 R[y mod m][x mod m] + 1 - m*m) * spread) / (2 m*m)) per pixel, [h, w] int64."""
    assert m in MATRICES and 0 <= spread <= 255
    R = bayer_rank(m)
    t = ((2 * R + 1 - m * m) * spread) // (2 * m * m)                       # // on int64 floors
    return t[(np.arange(h) % m)[:, None], (np.arange(w) % m)[None, :]]


def distances(img, pal_f32, lut_in, m, spread):
    """img [H,W,3] uint8 -> d [H,W,K] int64."""
    img = np.ascontiguousarray(img, np.uint8)
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3)
    assert pal.min() >= 0 and pal.max() <= 255 and pal.shape[0] <= 16
    C = np.trunc(pal).astype(np.int64)
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64)
    q = np.clip(c + perturbation(img.shape[0], img.shape[1], m, spread)[:, :, None], 0, 255)
    return ((q[:, :, None, :] - C[None, None, :, :]) ** 2).sum(-1)


def cells_indices(img, pal_f32, lut_in, cw, ch, k, fixed, groups, m, spread):
    """img [H,W,3] uint8 -> (the palette index per pixel [H,W] int64, the mask per cell [ceil(H/ch), ceil(W/cw)] uint16)."""
    assert cw in CELL_SIZES and ch in CELL_SIZES
    d = distances(img, pal_f32, lut_in, m, spread)
    h, w, K = d.shape
    cand = candidates(K, k, fixed, groups)
    member = np.array([[(s >> j) & 1 for j in range(K)] for s in cand], bool)          # [n_cand, K]
    big = np.int64(1) << 40
    idx = np.empty((h, w), np.int64)
    sets = np.empty((-(-h // ch), -(-w // cw)), np.uint16)
    for cy in range(sets.shape[0]):
        for cx in range(sets.shape[1]):
            dc = d[cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw].reshape(-1, K)       # the pixels inside the frame
            cost = np.concatenate([np.where(member[i:i + 512, None, :], dc[None], big).min(-1).sum(-1)
                                   for i in range(0, len(cand), 512)])                  # [n_cand] (in pieces: memory)
            best = int(np.argmin(cost))                                                 # the first of the least
            assert cost[best] < 1 << 26
            sets[cy, cx] = cand[best]
            pick = np.argmin(np.where(member[best][None], dc, big), axis=-1)            # the lowest j of the least
            idx[cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw] = pick.reshape(d[cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw].shape[:2])
    return idx, sets


def cells_u8(img, pal_f32, out_colors, lut_in, cw, ch, k, fixed, groups, m, spread):
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    idx, sets = cells_indices(img, pal_f32, lut_in, cw, ch, k, fixed, groups, m, spread)
    return out_colors[idx], sets


def cells_frames(frames, pal_f32, out_colors, lut_in, cw, ch, k, fixed, groups, m, spread):
    """frames [N,H,W,3] uint8 -> (out [N,H,W,3] uint8, sets [N, ceil(H/ch), ceil(W/cw)] uint16)."""
    res = [cells_u8(f, pal_f32, out_colors, lut_in, cw, ch, k, fixed, groups, m, spread) for f in frames]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
