"""Threshold matrices by the form the ordered kernels see them in, and two plain restatements (no GPU, no ctypes).

`thresholds_from_device_f32` (dither_pie_amd/csrc/host.cpp) derives from the values and the shape of a matrix
  * an integer form m / 2^sh, sh <= 13, only when every value is dyadic and in [0, 1] (otherwise float32 only);
  * pow2: both sizes are powers of two (positions by masking, otherwise by a float64 reciprocal);
  * a padded copy with rows of th_w + 3 entries (column x holds column x % th_w), only while th_h * (th_w + 3) <= 2^18;
  * class nibbles for power-of-two tables of at most 256 entries: bit q of nibble (r, p) says that with lane 0 at column p
    of row r none of the 64 lanes' pixel q (column p + 4 l + q) has a threshold below 1/2.
`host_form` restates those rules; CATALOGUE names one matrix per form and edge, each with the form it is meant to have, and the
import fails when a matrix does not have it.

`matrix_rule` restates MatrixDitherStrategy.dither in numpy float64 by brute force; `geometries` lists the frames and origins
both tiers run (tests/test_threshold_forms_cpu.py, tests/test_gpu_threshold_forms.py)."""
import numpy as np

PAD_LIMIT = 1 << 18      # entries of the padded copy
MAX_ENTRIES = 1 << 20    # dp_thresholds_create accepts no more
MAX_SHIFT = 13
ORIGIN_LIMIT = 1 << 30   # dp_ordered_u8: y0 + h and x0 + w may reach it


def host_form(m):
    """-> dict(sh, pow2, padded, tw_pad, nibbles): sh -1 without an integer form, tw_pad 0 without a padded copy, nibbles an
    int array [th_h, th_w] of 4-bit classes or None where the host computes none."""
    m = np.asarray(m)
    assert m.dtype == np.float32 and m.ndim == 2 and 1 <= m.size <= MAX_ENTRIES and not np.isnan(m).any()
    th_h, th_w = m.shape
    sh = -1
    if m.min() >= 0.0 and m.max() <= 1.0:
        v = m.astype(np.float64)
        for s in range(MAX_SHIFT + 1):
            if np.array_equal(v * float(1 << s), np.floor(v * float(1 << s))):
                sh = s
                break
    pow2 = (th_h & (th_h - 1)) == 0 and (th_w & (th_w - 1)) == 0
    padded = th_h * (th_w + 3) <= PAD_LIMIT
    nib = None
    if padded and pow2 and m.size <= 256:
        nib = np.zeros((th_h, th_w), np.int64)
        for r in range(th_h):
            for p0 in range(th_w):
                for q in range(4):
                    if all(m[r, (p0 + 4 * lane + q) % th_w] >= np.float32(0.5) for lane in range(64)):
                        nib[r, p0] |= 1 << q
    return dict(sh=sh, pow2=pow2, padded=padded, tw_pad=th_w + 3 if padded else 0, nibbles=nib)


def integer_table(m, sh):
    """The integer form of a matrix with one (host.cpp: m[i] = t * 2^sh)."""
    return (np.asarray(m, np.float64) * float(1 << sh)).astype(np.uint32)


def padded_rows(m):
    """The padded copy: th_w + 3 columns, column x from column x % th_w (th_w < 3: the pad wraps more than once)."""
    th_w = m.shape[1]
    return m[:, np.arange(th_w + 3) % th_w]


# ---------------------------------------------------------------------------------------------- the catalogue
def _dyadic(seed, shape, denom, force=()):
    """Random m / denom with m in 0 .. denom; `force`: values of m written over the first entries (row-major).  One forced odd
    m makes log2(denom) the smallest shift that holds the matrix."""
    m = np.random.RandomState(seed).randint(0, denom + 1, shape).astype(np.int64)
    m.reshape(-1)[:len(force)] = force
    return (m / float(denom)).astype(np.float32)


RUN = 70


def _classes(seed, th_h, th_w):
    """256 entries m / 256 on a power-of-two shape.  In row r the columns c with c % 4 == r % 4 hold values >= 1/2 only, each of
    the other three residue classes holds both sides of 1/2.  The 64 lanes of a wave that starts at column p meet, for pixel
    slot q, the columns of one residue class (all of them on every shape here): bit q of nibble (r, p) is set exactly when
    (p + q) % 4 == r % 4, so every nibble has one set and three clear bits and the set bit moves with the starting column.
    Rows of 128 columns and more begin with a run of RUN values >= 1/2: a rule that walked 64 consecutive columns instead of
    every fourth would set all four bits at the run's first columns, where the right rule finds an entry below 1/2 further on."""
    assert th_h * th_w == 256 and th_w % 4 == 0
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 256, (th_h, th_w)).astype(np.int64)
    for r in range(th_h):
        for c4 in range(4):
            cols = np.arange(c4, th_w, 4)
            if c4 == r % 4:
                m[r, cols] = rs.randint(128, 256, len(cols))
            else:
                m[r, cols[0]] = rs.randint(128, 256)      # one entry above 1/2 ...
                m[r, cols[-1]] = rs.randint(0, 128)       # ... and one below (behind the run), wherever the rest fell
    if th_w >= 128:
        m[:, :RUN] = rs.randint(128, 256, (th_h, RUN))
    m[0, 0] = 129                                         # an odd m: sh = 8
    return (m / 256.0).astype(np.float32)


def _catalogue():
    rs = np.random.RandomState(20240)
    cat = []

    def add(name, m, **form):
        cat.append((name, np.ascontiguousarray(m, np.float32), form))

    add("row1x7", (np.arange(7) / 7.0).reshape(1, 7), sh=-1, pow2=False, padded=True, tw_pad=10, cls=False)
    add("col5x1", (np.array([0, 3, 5, 8, 1]) / 8.0).reshape(5, 1), sh=3, pow2=False, padded=True, tw_pad=4, cls=False)
    add("m3x2", (np.array([[0, 9], [16, 5], [12, 3]]) / 16.0), sh=4, pow2=False, padded=True, tw_pad=5, cls=False)
    add("m2x3", (np.array([[7, 0, 14], [10, 16, 1]]) / 16.0), sh=4, pow2=False, padded=True, tw_pad=6, cls=False)
    add("cls4x64", _classes(1, 4, 64), sh=8, pow2=True, padded=True, tw_pad=67, cls=True)
    add("cls2x128", _classes(2, 2, 128), sh=8, pow2=True, padded=True, tw_pad=131, cls=True)
    add("cls1x256", _classes(3, 1, 256), sh=8, pow2=True, padded=True, tw_pad=259, cls=True)
    add("cls16x16", _classes(4, 16, 16), sh=8, pow2=True, padded=True, tw_pad=19, cls=True)
    add("int17x24", _dyadic(5, (17, 24), 256, [1]), sh=8, pow2=False, padded=True, tw_pad=27, cls=False)
    add("int64x32", _dyadic(6, (64, 32), 2048, [1]), sh=11, pow2=True, padded=True, tw_pad=35, cls=False)
    # the top of the uint32 decision d0 << 13 <= m * S: m = 0, 8191 and 8192 (t = 1.0 exactly) are in the table
    add("sh13_128x64", _dyadic(7, (128, 64), 8192, [0, 8191, 8192]), sh=13, pow2=True, padded=True, tw_pad=67, cls=False)
    add("int181x181", _dyadic(8, (181, 181), 256, [1]), sh=8, pow2=False, padded=True, tw_pad=184, cls=False)   # 133 KB of padded rows
    add("f33x20", rs.random_sample((33, 20)), sh=-1, pow2=False, padded=True, tw_pad=23, cls=False)
    add("outside6x10", rs.uniform(-0.25, 1.5, (6, 10)), sh=-1, pow2=False, padded=True, tw_pad=13, cls=False)
    add("pad_edge_1x262141", _dyadic(9, (1, 262141), 256, [1]), sh=8, pow2=False, padded=True, tw_pad=262144, cls=False)
    add("nopad_1x262142", _dyadic(9, (1, 262142), 256, [1]), sh=8, pow2=False, padded=False, tw_pad=0, cls=False)
    add("nopad512", rs.random_sample((512, 512)), sh=-1, pow2=True, padded=False, tw_pad=0, cls=False)
    add("nopad600x450", _dyadic(10, (600, 450), 1024, [1]), sh=10, pow2=False, padded=False, tw_pad=0, cls=False)
    add("max1024", _dyadic(11, (1024, 1024), 256, [1]), sh=8, pow2=True, padded=False, tw_pad=0, cls=False)
    return cat


CATALOGUE = _catalogue()
MATRICES = {name: m for name, m, _ in CATALOGUE}
CLAIMS = {name: form for name, _, form in CATALOGUE}
FORMS = {}


def check_catalogue():
    """Every matrix has the form it claims (run at import: an edit that loses a form fails here, not silently)."""
    for name, m, claim in CATALOGUE:
        f = host_form(m)
        FORMS[name] = f
        got = dict(sh=f["sh"], pow2=f["pow2"], padded=f["padded"], tw_pad=f["tw_pad"], cls=f["nibbles"] is not None and bool(f["nibbles"].any()))
        assert got == claim, (name, got, claim)
        if claim["cls"]:
            nib = f["nibbles"]
            assert (nib != 0).any() and (nib != 15).any(), name                       # a set bit and a clear bit
            assert all(len(set(nib[r].tolist())) > 1 for r in range(nib.shape[0])), name   # the bits differ between starting columns
    assert MATRICES["outside6x10"].min() < 0.0 and MATRICES["outside6x10"].max() > 1.0
    assert {0.0, 8191.0 / 8192.0, 1.0} <= set(MATRICES["sh13_128x64"].reshape(-1)[:3].tolist())
    e = MATRICES["pad_edge_1x262141"].shape
    assert e[0] * (e[1] + 3) == PAD_LIMIT and MATRICES["nopad_1x262142"].shape[1] == e[1] + 1
    assert MATRICES["max1024"].size == MAX_ENTRIES


check_catalogue()


# ---------------------------------------------------------------------------------------------- the matrix rule
def matrix_rule(arr, pal_f32, out_colors, lut_in, thr, y0, x0):
    """MatrixDitherStrategy.dither in numpy float64, with the uint8 / gamma wrapper around it as the oracle has it: the pixel's
    bytes (through lut_in) as float32, the squared distances to every palette entry by brute force, the two smallest as the
    re-squared square roots the KD-tree query returns, factor = nearest / total (0 where total == 0), nearest where
    factor <= float64(threshold at ((y0 + y) % th_h, (x0 + x) % th_w)), else second.

    -> (out uint8 [h, w, 3], undecided bool [h, w]).  A pixel is undecided when d0 == d1 or d1 == d2: which of two equally
    distant entries the tree reports first is its traversal order -- the oracle's business, not this function's."""
    arr = np.asarray(arr, np.uint8)
    h, w, _ = arr.shape
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3).astype(np.float64)
    K = pal.shape[0]
    src = arr if lut_in is None else np.asarray(lut_in, np.uint8)[arr]
    q = src.reshape(-1, 3).astype(np.float32).astype(np.float64)
    d = np.zeros((q.shape[0], K))
    for c in range(3):                                     # (dx^2 + dy^2) + dz^2, each square and sum rounded
        d += (q[:, c, None] - pal[None, :, c]) ** 2
    order = np.argsort(d, axis=1, kind="stable")[:, :3]
    rows = np.arange(q.shape[0])
    i0, i1 = order[:, 0], order[:, 1 if K > 1 else 0]
    d0, d1 = d[rows, i0], d[rows, i1]
    undecided = d0 == d1 if K > 1 else np.zeros(len(rows), bool)
    if K > 2:
        undecided |= d1 == d[rows, order[:, 2]]
    r0, r1 = np.sqrt(d0), np.sqrt(d1)
    s0, s1 = r0 * r0, r1 * r1
    total = s0 + s1
    factor = np.where(total == 0.0, 0.0, s0 / np.where(total == 0.0, 1.0, total))
    thr = np.asarray(thr)
    assert thr.dtype == np.float32 and thr.ndim == 2
    th_h, th_w = thr.shape
    ty = [(int(y0) + y) % th_h for y in range(h)]          # Python integers: no width to overflow
    tx = [(int(x0) + x) % th_w for x in range(w)]
    t = thr[np.asarray(ty)[:, None], np.asarray(tx)[None, :]].astype(np.float64).reshape(-1)
    pick = np.where(factor <= t, i0, i1)
    out = np.ascontiguousarray(out_colors, np.uint8).reshape(-1, 3)[pick].reshape(h, w, 3)
    return out, undecided.reshape(h, w)


# ---------------------------------------------------------------------------------------------- frames and origins
FRAME = (37, 131)


def geometries(thr_shape):
    """(h, w, y0, x0) of both tiers: the origin, a small one, one that puts the matrix's wrap inside the frame in both axes, the
    largest origin the entry point accepts, and one in the middle of the range."""
    th_h, th_w = thr_shape
    h, w = FRAME
    return [(h, w, 0, 0),
            (h, w, 5, 3),
            (h, w, (th_h - 20) % th_h, (th_w - 60) % th_w),
            (h, w, ORIGIN_LIMIT - h, ORIGIN_LIMIT - w),
            (h, w, (1 << 29) + 12345, (1 << 29) + 54321)]
