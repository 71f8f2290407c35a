"""numpy restatement of include/ditherpie_hip_scene.h and of the cut rule of dither_pie_amd/scenes.py -- written
independently of both, reads nothing but its arguments -- and the synthetic clips the scene tests share.

  signatures(frames)      np.bincount of the cell ids (r>>4)<<8 | (g>>4)<<4 | (b>>4) per frame -> int64 [N, 4096]
  distances(sig, prev)    int64 L1 of consecutive signatures; the first against `prev`, or 0 without one
  cut_starts(...)         the frames that start a scene, over a whole clip at once
  scene_ranges(n, starts) [(start, end)] tiling 0 ... n
"""
import numpy as np

BINS = 4096


def cell_ids(frames):
    f = np.asarray(frames, np.uint8).astype(np.int64)
    return ((f[..., 0] >> 4) << 8) | ((f[..., 1] >> 4) << 4) | (f[..., 2] >> 4)


def signatures(frames):
    f = np.asarray(frames, np.uint8)
    f = f.reshape((1,) + f.shape) if f.ndim == 3 else f
    ids = cell_ids(f).reshape(f.shape[0], -1)
    return np.stack([np.bincount(row, minlength=BINS) for row in ids]).astype(np.int64) if len(ids) else np.zeros((0, BINS), np.int64)


def distances(sig, prev=None):
    sig = np.asarray(sig, np.int64)
    out = np.zeros(len(sig), np.int64)
    if len(sig) > 1:
        out[1:] = np.abs(sig[1:] - sig[:-1]).sum(axis=1)
    if prev is not None and len(sig):
        out[0] = np.abs(sig[0] - np.asarray(prev, np.int64)).sum()
    return out


def cut_starts(dist, n_px, threshold, min_scene_frames):
    starts, last = [], 0
    for i in range(1, len(dist)):
        if int(dist[i]) > threshold * 2 * n_px and i - last >= min_scene_frames:
            starts.append(i)
            last = i
    return starts


def scene_ranges(n, starts):
    edges = [0] + list(starts) + [n]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


# ---------------------------------------------------------------------------------------------------- synthetic clips
H, W = 48, 64
LENGTHS = (15, 5, 20)          # three scenes, 40 frames; the middle one is shorter than the default min_scene_frames
MOVED = 300                    # pixels of the in-scene change: distance 2 * 300 = 600 < 0.4 * 2 * 3072
_RED = ((0, 80), (96, 160), (176, 256))   # the scenes' red ranges: disjoint 16^3 cells whatever green and blue are


def three_scene_clip(seed=5):
    """-> (frames uint8 [40, 48, 64, 3], moved frame numbers).  Within a scene every frame is a permutation of the scene's
    base frame (the same signature: distance 0) except ONE, in which MOVED pixels went to a cell no base pixel is in (green
    250; base frames keep green below 240) -- distance exactly 2 * MOVED to both neighbours.  The scenes share no cell:
    distance exactly 2 * H * W across a cut."""
    rs = np.random.RandomState(seed)
    frames, moved = [], []
    for k, n in enumerate(LENGTHS):
        base = np.stack([rs.randint(_RED[k][0], _RED[k][1], H * W), rs.randint(0, 240, H * W), rs.randint(0, 256, H * W)], axis=1).astype(np.uint8)
        special = 2 + k             # which frame of the scene carries the in-scene change (never its first or last)
        for i in range(n):
            f = base[rs.permutation(H * W)]
            if i == special:
                f = f.copy()
                f[rs.choice(H * W, MOVED, replace=False)] = (_RED[k][0] + 5, 250, 250)
                moved.append(len(frames))
            frames.append(f.reshape(H, W, 3))
    return np.stack(frames), moved
