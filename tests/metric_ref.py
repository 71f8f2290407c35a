"""The Oklab colour metric as include/ditherpie_hip_metric.h defines it, in numpy: the plain statement the host code and the
GPU kernels are held to.  All integer arithmetic (>> floors); only the ordered decision divides, in IEEE float64.

  LIN[v]   = round(65535 f(v / 255)), f the sRGB decoding function        (the literal below; test_metric_cpu checks it)
  (l,m,s)  = (A . (LIN[r], LIN[g], LIN[b])) >> 16                          unsigned 32-bit products
  c        = floor(cbrt(x * 2^32)) per component                           exact, 0 .. 65535
  (L,a,b)  = (B . (cl, cm, cs)) >> 14                                      signed 32-bit sums
  d(q, k)  = dL^2 + da^2 + db^2
  nearest, second = the two smallest (d(q, k), k), compared as pairs: the lowest index wins on equal distance; K = 1: both 0
  ordered  : f = d0 / (d0 + d1) (0 when the sum is 0); the pixel takes nearest iff f <= float64(t), else second

With metric "rgb" lab() is the identity on the bytes: top2() is then the squared Euclidean RGB distance under the same pair
order (what dp_metric_top2_host computes for metric 0; NOT scipy's tie order).

NearestAdapter stands in for the CPU oracle where tests/pattern_ref.py and tests/dotdiff_ref.py call
orc.ordered_u8(t, pal_f32, out_colors, None, "none", want_idx=True): passing it turns those two files into the statement of
pattern dithering and dot diffusion on a metric palette."""
import numpy as np

LIN = np.array([
    0, 20, 40, 60, 80, 99, 119, 139, 159, 179, 199, 219, 241, 264, 288, 313,
    340, 367, 396, 427, 458, 491, 526, 562, 599, 637, 677, 718, 761, 805, 851, 898,
    947, 997, 1048, 1101, 1156, 1212, 1270, 1330, 1391, 1453, 1517, 1583, 1651, 1720, 1790, 1863,
    1937, 2013, 2090, 2170, 2250, 2333, 2418, 2504, 2592, 2681, 2773, 2866, 2961, 3058, 3157, 3258,
    3360, 3464, 3570, 3678, 3788, 3900, 4014, 4129, 4247, 4366, 4488, 4611, 4736, 4864, 4993, 5124,
    5257, 5392, 5530, 5669, 5810, 5953, 6099, 6246, 6395, 6547, 6700, 6856, 7014, 7174, 7335, 7500,
    7666, 7834, 8004, 8177, 8352, 8528, 8708, 8889, 9072, 9258, 9445, 9635, 9828, 10022, 10219, 10417,
    10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909,
    14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001,
    18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721,
    23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094,
    28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143,
    34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891,
    41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359,
    48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567,
    57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535,
], np.int64)
A = np.array([[27015, 35149, 3372], [13887, 44611, 7038], [5787, 18463, 41286]], np.int64)
B = np.array([[862, 3251, -17], [8102, -9948, 1846], [106, 3206, -3312]], np.int64)
METRICS = ("rgb", "oklab")


def lin_formula():
    """LIN from its formula, in float64 (no value lies closer than 0.0016 to a rounding boundary)."""
    u = np.arange(256) / 255.0
    f = np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)
    return np.floor(65535.0 * f + 0.5).astype(np.int64)


def icbrt32(x):
    """floor(cbrt(x * 2^32)) for integers 0 <= x < 2^16, exactly: a float estimate corrected in integers."""
    x = np.asarray(x, np.int64)
    big = x << 32
    c = np.floor(np.cbrt(big.astype(np.float64))).astype(np.int64)
    for _ in range(2):
        c = np.where(c * c * c > big, c - 1, c)
        c = np.where((c + 1) ** 3 <= big, c + 1, c)
    assert np.all(c ** 3 <= big) and np.all((c + 1) ** 3 > big) and c.min() >= 0 and c.max() <= 65535
    return c


_CBRT = None


def lab(rgb, metric="oklab"):
    """uint8 [..., 3] -> int32 [..., 3]: (L, a, b), or the bytes themselves under "rgb"."""
    global _CBRT
    rgb = np.asarray(rgb)
    assert rgb.shape[-1] == 3 and metric in METRICS
    if metric == "rgb":
        return rgb.astype(np.int32)
    if _CBRT is None:
        _CBRT = icbrt32(np.arange(65536))
    lin = LIN[rgb.astype(np.int64)]
    lms = (lin @ A.T) >> 16
    assert lms.size == 0 or (lms.min() >= 0 and lms.max() <= 65535)
    return ((_CBRT[lms] @ B.T) >> 14).astype(np.int32)


def palette_bytes(pal_f32):
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3)
    assert 1 <= pal.shape[0] <= 256 and np.array_equal(pal, np.floor(pal)) and pal.min() >= 0 and pal.max() <= 255
    return pal.astype(np.uint8)


def top2(rgb, pal_f32, metric="oklab", want_d=False):
    """rgb uint8 [..., 3] -> (nearest, second) int64 [...] (and their distances, int64)."""
    rgb = np.asarray(rgb, np.uint8)
    shape = rgb.shape[:-1]
    q = lab(rgb.reshape(-1, 3), metric).astype(np.int64)
    p = lab(palette_bytes(pal_f32), metric).astype(np.int64)
    K, n = p.shape[0], q.shape[0]
    i0, i1, d0, d1 = (np.zeros(n, np.int64) for _ in range(4))
    rows = np.arange(1 << 16)
    for s in range(0, n, 1 << 16):
        e = min(n, s + (1 << 16))
        d = ((q[s:e, None, :] - p[None, :, :]) ** 2).sum(-1)              # [m, K]
        r = rows[:e - s]
        a = np.argmin(d, axis=1)                                         # the first minimum: the lowest index
        i0[s:e], d0[s:e] = a, d[r, a]
        if K > 1:
            d2 = d.copy()
            d2[r, a] = 1 << 62
            b = np.argmin(d2, axis=1)
            i1[s:e], d1[s:e] = b, d[r, b]
        else:
            d1[s:e] = d0[s:e]
    out = (i0.reshape(shape), i1.reshape(shape))
    return out + (d0.reshape(shape), d1.reshape(shape)) if want_d else out


def ordered_indices(img, pal_f32, thr=None, y0=0, x0=0, metric="oklab"):
    """img uint8 [H,W,3] or [N,H,W,3] -> the chosen palette index per pixel (int64).  thr None: nearest only."""
    img = np.asarray(img, np.uint8)
    i0, i1, d0, d1 = top2(img, pal_f32, metric, want_d=True)
    if thr is None:
        return i0
    thr = np.asarray(thr)
    assert thr.dtype == np.float32 and thr.ndim == 2
    h, w = img.shape[-3], img.shape[-2]
    t = thr[((y0 + np.arange(h)) % thr.shape[0])[:, None], ((x0 + np.arange(w)) % thr.shape[1])[None, :]].astype(np.float64)
    s = (d0 + d1).astype(np.float64)
    f = np.where(s > 0, d0.astype(np.float64) / np.where(s > 0, s, 1.0), 0.0)
    return np.where(f <= t, i0, i1)


def ordered_u8(img, pal, out_colors, thr=None, y0=0, x0=0, metric="oklab"):
    """img uint8 [H,W,3] or [N,H,W,3] -> the dithered image, out_colors[index]."""
    out_colors = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)
    return out_colors[ordered_indices(img, pal, thr, y0, x0, metric)]


class NearestAdapter:
    """The one method pattern_ref / dotdiff_ref call on their `orc`, answering under the metric."""

    def __init__(self, metric="oklab"):
        self.metric = metric

    def ordered_u8(self, img, pal_f32, out_colors, thr, mode, want_idx=False):
        assert thr is None and mode == "none"
        idx = top2(img, pal_f32, self.metric)[0]
        out = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)[idx]
        return (out, idx) if want_idx else out
