"""Integer error diffusion as include/ditherpie_hip_idiff.h defines it, in numpy / Python: the plain PUSH-form statement the GPU
kernel (a pull form on an anti-diagonal schedule) is held to.  All integer arithmetic.  nearest() is what the `orc` adapter
answers for a nearest-only search (oracle.ordered_u8(..., None, "none", want_idx=True): scipy's KD-tree order on ties, no lut_in;
metric_ref.NearestAdapter under the Oklab metric), memoised on the query within a call: the scan is serial."""
import numpy as np

# the reference's eight tap sets (dithering_lib.ErrorDiffusionKernel): (dx, dy, weight) lists and divisors
KERNELS = {
    "floyd_steinberg": ([(1, 0, 7), (-1, 1, 3), (0, 1, 5), (1, 1, 1)], 16),
    "jjn": ([(1, 0, 7), (2, 0, 5)] + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (3, 5, 7, 5, 3))]
            + [(dx, 2, wt) for dx, wt in zip(range(-2, 3), (1, 3, 5, 3, 1))], 48),
    "stucki": ([(1, 0, 8), (2, 0, 4)] + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 8, 4, 2))]
               + [(dx, 2, wt) for dx, wt in zip(range(-2, 3), (1, 2, 4, 2, 1))], 42),
    "burkes": ([(1, 0, 8), (2, 0, 4)] + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 8, 4, 2))], 32),
    "atkinson": ([(1, 0, 1), (2, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1), (0, 2, 1)], 8),
    "sierra": ([(1, 0, 5), (2, 0, 3)] + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 5, 4, 2))]
               + [(dx, 2, wt) for dx, wt in zip(range(-1, 2), (2, 3, 2))], 32),
    "sierra_two_row": ([(1, 0, 4), (2, 0, 3)] + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (1, 2, 3, 2, 1))], 16),
    "sierra_lite": ([(1, 0, 2), (-1, 1, 1), (0, 1, 1)], 4),
}
MAX_TAPS = 12


def check_taps(taps, divisor, strength256):
    """The rules of the header; ValueError names the first one broken."""
    taps = [tuple(int(v) for v in t) for t in taps]
    if not 1 <= len(taps) <= MAX_TAPS:
        raise ValueError("n_taps")
    if divisor < 1:
        raise ValueError("divisor")
    if not 0 <= strength256 <= 256:
        raise ValueError("strength256")
    for dx, dy, wt in taps:
        if not (0 <= dy <= 2 and -2 <= dx <= 2 and (dy > 0 or dx >= 1)):
            raise ValueError("window")
        if wt < 0:
            raise ValueError("weight")
    if len({(dx, dy) for dx, dy, _ in taps}) != len(taps):
        raise ValueError("twice")
    if sum(wt for _, _, wt in taps) > divisor:
        raise ValueError("sum")
    return taps


def shares(taps, divisor, strength256):
    """q_k = floor(weight_k * strength256 * 256 / divisor)."""
    return [wt * strength256 * 256 // divisor for _, _, wt in check_taps(taps, divisor, strength256)]


def skew(taps):
    """The smallest s >= 1 with s * dy + dx >= 1 for every tap with dy >= 1."""
    s = 1
    while any(dy >= 1 and s * dy + dx < 1 for dx, dy, _ in taps):
        s += 1
    return s


WINDOW = [(1, 0), (2, 0)] + [(dx, dy) for dy in (1, 2) for dx in range(-2, 3)]   # the 12 positions a tap may take
N_RANDOM_CASES = 12


def tap_cases():
    """A fixed list of (taps, divisor, strength256) beyond the eight variants: what the plan accepts and no named variant has.
    The first part is written by hand; N_RANDOM_CASES sets from numpy.random.RandomState(7) follow (a random subset of WINDOW
    in window order, weights 0 .. 8, the divisor their sum plus 0 .. 2 and at least 1, strength 256)."""
    cases = [
        ([(1, 0, 1)], 1, 256),                                          # one tap: the whole error goes right, nothing leaves a row
        ([(2, 0, 1)], 1, 256),                                          # no dx = 1 tap: two interleaved chains per row
        ([(0, 1, 1)], 1, 256),                                          # straight down, skew 1: columns never meet
        ([(0, 2, 1)], 1, 256),                                          # rows 0 and 1 of a band read only the two rows above it
        ([(-1, 2, 1)], 1, 256),                                         # skew 1 with a left-pointing tap: finished one step earlier
        ([(-2, 2, 1)], 1, 256),                                         # skew 2 from a dy = 2 tap alone
        ([(-2, 1, 1)], 1, 256),                                         # skew 3 from one tap
        ([(-2, 1, 1), (2, 2, 1)], 2, 256),                              # skew * dy + dx = 8, the ring depth, in the 4-slot instance
        ([(1, 0, 7), (0, 1, 5), (1, 1, 3), (0, 2, 1)], 16, 256),        # skew 1 with four taps: no spare slot
        ([(2, 1, 1), (2, 2, 1)], 2, 256),                               # no (1, 0) tap, skew 1, both taps reach past the row's end
        ([(1, 0, 5), (2, 0, 3), (-1, 1, 2), (0, 1, 4), (1, 2, 2)], 16, 256),   # 5 taps: the 7-slot instance with two spare slots
        ([(2, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1), (0, 2, 1), (2, 2, 1)], 8, 256),   # 6 taps, no (1, 0), a quarter dropped
        ([(1, 0, 4), (2, 0, 3), (0, 1, 3), (1, 1, 2), (2, 1, 1), (0, 2, 2), (1, 2, 1)], 16, 256),   # 7 taps at skew 1: no spare slot
        ([(1, 0, 4), (2, 0, 2), (0, 1, 4), (1, 1, 2), (2, 1, 1), (-1, 2, 1), (0, 2, 1), (1, 2, 1)], 16, 256),   # 8 taps at skew 1: 12 slots
        ([(1, 0, 4), (2, 0, 2), (-1, 1, 2), (0, 1, 4), (1, 1, 2), (2, 1, 1), (-1, 2, 1), (0, 2, 2), (1, 2, 1)], 20, 256),   # 9 taps, skew 2
        ([(1, 0, 8), (2, 0, 4), (-1, 1, 4), (0, 1, 8), (1, 1, 4), (2, 1, 2), (-2, 2, 1), (-1, 2, 2), (0, 2, 4), (1, 2, 2)], 42, 256),   # 10, skew 2
        ([t for t in KERNELS["jjn"][0] if t[:2] != (-2, 2)], 48, 256),  # 11 taps: one spare slot of the 12-slot instance, skew 3
        ([(dx, dy, 1) for dx, dy in WINDOW], 12, 256),                  # all 12 positions with equal weights
        ([(1, 0, 7), (0, 1, 5), (1, 1, 4), (-2, 1, 0)], 16, 256),       # a zero-weight tap: it raises the skew to 3 and moves nothing
        ([(1, 0, 1), (0, 1, 1), (1, 1, 1)], 1000, 256),                 # weights summing to 3 over 1000: shares of 65 / 65536
        (KERNELS["floyd_steinberg"][0], 16, 255),                       # strength 255: every share one 256th short
    ]
    rs = np.random.RandomState(7)
    for _ in range(N_RANDOM_CASES):
        n = int(rs.randint(1, MAX_TAPS + 1))
        where = sorted(rs.permutation(len(WINDOW))[:n].tolist())
        weights = rs.randint(0, 9, n).tolist()
        divisor = max(1, sum(weights) + int(rs.randint(0, 3)))
        cases.append(([WINDOW[p] + (wt,) for p, wt in zip(where, weights)], divisor, 256))
    return cases


def idiff_indices(orc, img, pal_f32, out_colors, lut_in, taps, divisor, strength256, want_acc=False):
    """img [H,W,3] uint8 -> the chosen palette index per pixel [H,W] (int64) (and the largest |acc| seen)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, _ = img.shape
    pal_f32 = np.ascontiguousarray(pal_f32, np.float32).reshape(-1, 3)
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    assert 1 <= pal_f32.shape[0] <= 256 and pal_f32.min() >= 0 and pal_f32.max() <= 255
    taps = check_taps(taps, divisor, strength256)
    q = shares(taps, divisor, strength256)
    C = np.trunc(pal_f32).astype(np.int64).tolist()
    c = (np.asarray(lut_in, np.uint8)[img] if lut_in is not None else img).astype(np.int64).tolist()
    acc = [[[0, 0, 0] for _ in range(w)] for _ in range(h)]
    idx = np.zeros((h, w), np.int64)
    memo = {}
    big = 0
    for y in range(h):
        for x in range(w):
            a = acc[y][x]
            big = max(big, abs(a[0]), abs(a[1]), abs(a[2]))
            u = [min(max(16 * c[y][x][ch] + a[ch], 0), 4080) for ch in range(3)]
            t = ((u[0] + 8) >> 4, (u[1] + 8) >> 4, (u[2] + 8) >> 4)
            k = memo.get(t)
            if k is None:
                k = memo[t] = int(orc.ordered_u8(np.array(t, np.uint8).reshape(1, 1, 3), pal_f32, out_colors, None, "none",
                                                 want_idx=True)[1].reshape(-1)[0])
            idx[y, x] = k
            e = [u[ch] - 16 * C[k][ch] for ch in range(3)]
            for (dx, dy, _), qk in zip(taps, q):
                ny, nx = y + dy, x + dx
                if ny < h and 0 <= nx < w:
                    d = acc[ny][nx]
                    for ch in range(3):
                        s = (abs(e[ch]) * qk) >> 16                    # trunc toward zero, no division
                        d[ch] += s if e[ch] >= 0 else -s
    return (idx, big) if want_acc else idx


def idiff_u8(orc, img, pal_f32, out_colors, lut_in, taps, divisor, strength256):
    """img [H,W,3] uint8 -> the dithered image [H,W,3] uint8."""
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    return out_colors[idiff_indices(orc, img, pal_f32, out_colors, lut_in, taps, divisor, strength256)]


def idiff_frames(orc, frames, pal_f32, out_colors, lut_in, taps, divisor, strength256):
    return np.stack([idiff_u8(orc, f, pal_f32, out_colors, lut_in, taps, divisor, strength256) for f in frames])
