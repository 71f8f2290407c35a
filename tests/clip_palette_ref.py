"""numpy restatement of the two device pieces of include/ditherpie_hip_clip.h: the distinct colours of a stream of pixel
buffers in order of first occurrence, and the rank sample of a colour histogram.  Written for clarity, checked against
brute-force Python on tiny inputs by tests/test_clip_palette_cpu.py; the GPU tests compare the kernels with it."""
import numpy as np


def _codes(px):
    px = np.asarray(px, np.uint8).reshape(-1, 3).astype(np.int64)
    return px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)


def distinct_first(px):
    """The distinct rows of uint8 [n,3] in order of first occurrence."""
    px = np.asarray(px, np.uint8).reshape(-1, 3)
    _, first = np.unique(_codes(px), return_index=True)
    return px[np.sort(first)]


class DistinctStream:
    """add(px) appends the colours of px that no earlier add has seen, in order of first occurrence within px."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.seen = np.zeros(1 << 24, bool)
        self.list = np.zeros((0, 3), np.uint8)

    def add(self, px):
        px = np.asarray(px, np.uint8).reshape(-1, 3)
        if len(px):
            d = distinct_first(px)
            new = d[~self.seen[_codes(d)]]
            self.seen[_codes(new)] = True
            self.list = np.concatenate([self.list, new])
        return self

    def colours(self):
        return self.list


def slot_of(px):
    """The histogram's slot of every pixel: (r>>4)<<20 | (g>>4)<<16 | (b>>4)<<12 | (r&15)<<8 | (g&15)<<4 | (b&15)."""
    px = np.asarray(px, np.uint8).reshape(-1, 3).astype(np.int64)
    r, g, b = px[:, 0], px[:, 1], px[:, 2]
    return ((r >> 4) << 20) | ((g >> 4) << 16) | ((b >> 4) << 12) | ((r & 15) << 8) | ((g & 15) << 4) | (b & 15)


def colour_of(slot):
    slot = np.asarray(slot, np.int64)
    r = ((slot >> 20) & 15) << 4 | ((slot >> 8) & 15)
    g = ((slot >> 16) & 15) << 4 | ((slot >> 4) & 15)
    b = ((slot >> 12) & 15) << 4 | (slot & 15)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def histogram(px):
    """count[slot] over all 2^24 slots (int64)."""
    return np.bincount(slot_of(px), minlength=1 << 24).astype(np.int64)


def rank_sample(hist, ranks):
    """-> (uint8 [n,3], number of ranks outside [0, total)): the colour of the pixel of each zero-based rank when the
    histogram's pixels are laid out in slot order, every colour count times; out-of-range ranks give (0, 0, 0)."""
    hist = np.asarray(hist, np.int64)
    ranks = np.asarray(ranks, np.int64).reshape(-1)
    ends = np.cumsum(hist)                       # ends[s] = pixels in slots <= s
    total = int(ends[-1]) if len(ends) else 0
    ok = (ranks >= 0) & (ranks < total)
    slot = np.searchsorted(ends, np.where(ok, ranks, 0), side="right")   # the first slot whose end passes the rank
    out = colour_of(np.minimum(slot, (1 << 24) - 1))
    out[~ok] = 0
    return out, int((~ok).sum())
