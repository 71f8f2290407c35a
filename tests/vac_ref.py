"""The normative numpy statement of the void-and-cluster generator of include/ditherpie_hip_voidcluster.h (Ulichney 1993 on a
torus, all integer): mix32, weights, ranks, thresholds, and lowfreq, the low-frequency share of a binarised matrix's power.
Test infrastructure: imported by the tests of both tiers, never by the package."""
import math

import numpy as np

MIN_SIZE, MAX_SIZE = 8, 128
MIN_SIGMA256, MAX_SIGMA256, DEFAULT_SIGMA256 = 256, 768, 384
GREYS = (0.1, 0.25, 0.5, 0.75, 0.9)


def mix32(x):
    x = int(x) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def key(i, seed):
    return mix32(mix32(i) ^ (int(seed) & 0xffffffff))


def weights(sigma256):
    """W[d2] for d2 = 0 .. D, D the last squared distance of a non-zero weight."""
    W = []
    d2 = 0
    while True:
        v = int(math.floor(math.exp(-(d2 * 32768.0) / (sigma256 * sigma256)) * 1048576.0 + 0.5))
        if v == 0:
            return np.array(W, np.int64)
        W.append(v)
        d2 += 1


def cell_weights(h, w, sigma256):
    """T(0, q) for every cell q: the minimum image on the torus, counted once, whatever the window's width."""
    W = weights(sigma256)
    a = np.minimum(np.arange(h), h - np.arange(h))[:, None]
    b = np.minimum(np.arange(w), w - np.arange(w))[None, :]
    d2 = a * a + b * b
    return np.where(d2 < len(W), W[np.minimum(d2, len(W) - 1)], 0).astype(np.int64)


def ranks(h, w, seed, sigma256=DEFAULT_SIGMA256, info=None):
    """Rank matrix [h, w], int64, a permutation of 0 .. h*w-1.  info (a dict) receives the number of relaxation rounds."""
    assert MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE and MIN_SIGMA256 <= sigma256 <= MAX_SIGMA256
    n = h * w
    T = cell_weights(h, w, sigma256)
    BIG = np.int64(1) << 40
    E = np.zeros((h, w), np.int64)
    on = np.zeros((h, w), bool)

    def flip(p, sign):
        y, x = divmod(int(p), w)
        E[:] += sign * np.roll(T, (y, x), (0, 1))
        on[y, x] = sign > 0

    def tightest():
        return int(np.where(on, E, -1).argmax())          # argmax / argmin return the first: the lowest row-major index

    def emptiest():
        return int(np.where(on, BIG, E).argmin())

    n1 = max(1, n // 10)
    order = sorted(range(n), key=lambda i: (key(i, seed), i))
    for i in order[:n1]:
        flip(i, +1)
    rounds, done = 0, False
    while rounds < 4 * n and not done:
        c = tightest()
        flip(c, -1)
        v = emptiest()
        flip(v, +1)
        rounds += 1
        done = v == c
    if info is not None:
        info["rounds"], info["converged"] = rounds, done
    proto = on.copy()
    rank = np.full(n, -1, np.int64)
    for r in range(n1 - 1, -1, -1):
        c = tightest()
        flip(c, -1)
        rank[c] = r
    assert not on.any() and not E.any()                   # integer weights: nothing is left of the energy
    for i in np.flatnonzero(proto):
        flip(i, +1)
    for r in range(n1, n):
        v = emptiest()
        flip(v, +1)
        rank[v] = r
    return rank.reshape(h, w)


def thresholds(rank):
    """float32 thresholds of a rank matrix: the centres of min(n, 4096) equal bins of (0, 1)."""
    n = rank.size
    L = min(n, 4096)
    level = rank.astype(np.int64) * L // n
    return ((2 * level + 1).astype(np.float64) / (2 * L)).astype(np.float32)


def lowfreq(rank, grey):
    """The pattern rank < grey * n: mean power below a quarter of Nyquist over mean power at all non-zero frequencies."""
    h, w = rank.shape
    pat = (rank < grey * rank.size).astype(np.float64)
    P = np.abs(np.fft.fft2(pat - pat.mean())) ** 2
    f = np.hypot(np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :])
    return float(P[(f > 0) & (f < 0.125)].mean() / P[f > 0].mean())
