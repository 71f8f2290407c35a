"""Oklab palette fitting as include/ditherpie_hip_okfit.h defines it, in numpy: the plain statement dp_okfit_host and the GPU
kernels are held to.  All integer arithmetic, // floors; no random numbers; a pure function of the colour multiset.

  points    the n distinct colours in ascending order of code = r << 16 | g << 8 | b, count[i] >= 1, P[i] = metric_ref.lab(colour i)
  d         dL^2 + da^2 + db^2 (int64 here; at most 408 098 306)
  seeding   centre 0 = P of the point with the largest count (the lowest code on ties); centre j = P of the point that maximises
            count[i] * dmin[i] (uint64; the lowest code on ties), dmin the distance to the nearest centre chosen so far; a maximum
            of 0 repeats centre 0
  Lloyd     at most max_iter times: every point takes the centre of least d (the lowest index on ties); a centre with members
            becomes (2 S + cnt) // (2 cnt) per component, S = sum count * P, cnt = sum count; one without keeps its value; stop
            when no centre changed.  n_iter counts the assignment passes.
  bytes     one more assignment against the final centres; entry k is the colour of the member of k nearest to centre k (the
            lowest code on ties), a centre without members searches all points
  returns   palette uint8 [K, 3], centres int32 [K, 3], n_iter, distortion = sum count * d(point, its centre) of that last assignment

`metric` "rgb" runs the same algorithm on the bytes (metric_ref.lab's identity): what test_okfit_cpu compares the fit with."""
import json
import os

import numpy as np

import metric_ref as mr

MAX_K = 256
MAX_ITER = 10000


def points_of(pixels):
    """uint8 [..., 3] -> (codes uint32 ascending, counts int64): the colour multiset."""
    px = np.asarray(pixels, np.uint8).reshape(-1, 3).astype(np.uint32)
    codes, counts = np.unique(px[:, 0] << 16 | px[:, 1] << 8 | px[:, 2], return_counts=True)
    return codes.astype(np.uint32), counts.astype(np.int64)


def colours_of(codes):
    c = np.asarray(codes, np.int64)
    return np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)


def _check(codes, counts, K, max_iter):
    codes = np.asarray(codes, np.int64).reshape(-1)
    counts = np.asarray(counts, np.int64).reshape(-1)
    if not (1 <= K <= MAX_K and 1 <= max_iter <= MAX_ITER and len(codes) == len(counts) >= 1):
        raise ValueError("1 <= K <= 256, 1 <= max_iter <= 10000, n >= 1")
    if codes.min() < 0 or codes.max() >= 1 << 24 or np.any(np.diff(codes) <= 0) or counts.min() < 1 or int(counts.sum()) >= 1 << 32:
        raise ValueError("codes ascending and below 2^24, counts >= 1, their sum below 2^32")
    return codes, counts


def _dist(P, C):
    return ((P[:, None, :] - C[None, :, :]) ** 2).sum(-1)                  # [n, K] int64


def seed(P, counts, K):
    """The greedy k-means++ centres -> int64 [K, 3]."""
    C = np.zeros((K, 3), np.int64)
    C[0] = P[int(np.argmax(counts))]                                      # argmax: the first maximum, the lowest code
    dmin = None
    for j in range(1, K):
        d = ((P - C[j - 1]) ** 2).sum(-1)
        dmin = d if dmin is None else np.minimum(dmin, d)
        prod = counts * dmin                                              # < 2^32 * 2^29: exact in int64
        i = int(np.argmax(prod))
        C[j] = P[i] if prod[i] > 0 else C[0]
    return C


def assign(P, C):
    d = _dist(P, C)
    lab = np.argmin(d, axis=1)                                            # the first minimum: the lowest centre index
    return lab, d[np.arange(len(P)), lab]


def distortion(P, counts, C):
    return int((counts * assign(P, C)[1]).sum())


def fit_points(codes, counts, K, max_iter=100, metric="oklab", want_seed=False):
    codes, counts = _check(codes, counts, int(K), int(max_iter))
    P = mr.lab(colours_of(codes), metric).astype(np.int64)
    C = seed(P, counts, K)
    C_seed = C.copy()
    n_iter = 0
    for _ in range(max_iter):
        n_iter += 1
        lab, _ = assign(P, C)
        new = C.copy()
        for k in np.unique(lab):
            m = lab == k
            cnt = int(counts[m].sum())
            S = (counts[m, None] * P[m]).sum(0)
            new[k] = (2 * S + cnt) // (2 * cnt)                           # numpy's // floors
        same = np.array_equal(new, C)
        C = new
        if same:
            break
    lab, d = assign(P, C)
    pal = np.zeros((K, 3), np.uint8)
    for k in range(K):
        m = np.nonzero(lab == k)[0]
        if len(m):
            i = m[int(np.argmin(d[m]))]                                   # ascending codes: the first minimum is the lowest code
        else:
            i = int(np.argmin(((P - C[k]) ** 2).sum(-1)))
        pal[k] = colours_of(codes[i])
    out = (pal, C.astype(np.int32), n_iter, int((counts * d).sum()))
    return out + (C_seed.astype(np.int32),) if want_seed else out


def fit(pixels, K, max_iter=100, metric="oklab", want_seed=False):
    """uint8 [..., 3] -> (palette, centres, n_iter, distortion)."""
    return fit_points(*points_of(pixels), K, max_iter, metric, want_seed)


# ------------------------------------------------------------------------------------------------------- the shared cases
SAME_LAB = ((0, 194, 112), (1, 194, 112))                          # two colours, one Lab (11716, -2623, 1218): 2224 such pairs in the cube
EQUIDISTANT = ((144, 73, 8), (121, 178, 217), (228, 148, 212))      # p, A, B: d(lab p, lab A) == d(lab p, lab B) = 27 996 362
HALF_WAY = ((0, 100, 200), (0, 100, 255))                          # Labs (8430, -701, -2769), (9169, -618, -3934): every sum is odd


def code_of(rgb):
    return (int(rgb[0]) << 16) | (int(rgb[1]) << 8) | int(rgb[2])


def random_points(n, seed, max_count=1000):
    """n distinct random colours with counts in [1, max_count] -> (codes, counts)."""
    rs = np.random.RandomState(seed)
    codes = np.unique(rs.randint(0, 1 << 24, n + n // 4 + 8).astype(np.uint32))
    assert len(codes) >= n
    codes = np.sort(rs.permutation(codes)[:n])
    return codes.astype(np.uint32), rs.randint(1, max_count + 1, n).astype(np.int64)


def _pts(colours, counts):
    codes = np.array([code_of(c) for c in colours], np.uint32)
    order = np.argsort(codes)
    return codes[order], np.asarray(counts, np.int64)[order]


def emptied_centre_case():
    """tests/golden/okfit_emptied_centre.json: greys and counts on which a centre loses every member in a later pass."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "okfit_emptied_centre.json")) as f:
        rec = json.load(f)
    return _pts([(g, g, g) for g in rec["greys"]], rec["counts"]) + (int(rec["K"]), 100)


def lloyd_trace(codes, counts, K, max_iter=100):
    """The member counts (points, not pixels) of every centre in every assignment pass of the Lloyd loop -> int64 [n_iter, K]."""
    codes, counts = _check(codes, counts, K, max_iter)
    P = mr.lab(colours_of(codes)).astype(np.int64)
    C = seed(P, counts, K)
    rows = []
    for _ in range(max_iter):
        lab, _ = assign(P, C)
        rows.append(np.bincount(lab, minlength=K))
        new = C.copy()
        for k in np.unique(lab):
            m = lab == k
            cnt = int(counts[m].sum())
            new[k] = (2 * (counts[m, None] * P[m]).sum(0) + cnt) // (2 * cnt)
        same = np.array_equal(new, C)
        C = new
        if same:
            break
    return np.array(rows)


def cases():
    """name -> (codes, counts, K, max_iter): the cases the host statement (tests/test_okfit_cpu.py) and the kernels
    (tests/test_gpu_okfit.py) are both held to."""
    out = {}
    one = _pts([(12, 200, 77)], [5])
    out["n1_k1"] = one + (1, 100)
    out["n1_k3_duplicates"] = one + (3, 100)
    out["n5_k16_duplicates"] = random_points(5, 1) + (16, 100)
    out["n16_k16"] = random_points(16, 2) + (16, 100)
    for K in (1, 2, 16, 17, 255, 256):
        out[f"n300_k{K}"] = random_points(300, 10 + K) + (K, 100)
    a, b = SAME_LAB
    far = (255, 255, 255)
    out["same_lab_code_order_decides"] = _pts([a, b, far], [7, 7, 3]) + (2, 100)          # a and b tie for centre 0: the lower code
    out["same_lab_k3_repeats_centre_0"] = _pts([a, b, far], [7, 7, 3]) + (3, 100)        # only two distinct Labs: centre 2 = centre 0
    p, A, B = EQUIDISTANT
    out["equidistant_centre_index_decides"] = _pts([p, A, B], [1, 1000, 900]) + (2, 1)   # centres A, B; p is as far from both
    out["huge_count"] = _pts([(1, 2, 3), (250, 120, 30)], [(1 << 32) - 2, 1]) + (2, 100)
    out["huge_count_k1"] = _pts([(1, 2, 3), (250, 120, 30)], [1, (1 << 32) - 2]) + (1, 100)
    out["max_iter_1"] = random_points(300, 3) + (16, 1)
    out["max_iter_2"] = random_points(300, 3) + (16, 2)
    out["half_way_negative_mean"] = _pts(list(HALF_WAY), [1, 1]) + (1, 100)
    out["half_way_negative_mean_weighted"] = _pts(list(HALF_WAY) + [(0, 140, 230)], [3, 2, 1]) + (1, 100)
    out["emptied_centre"] = emptied_centre_case()
    return out
