"""What the tests of the two-level fine table share (dither_pie_amd/csrc/host_logic.h: fine_pack_sub; ordered_fine.h: fine_sub_level):
the numbering of cells and sub-cells, brute-force sets, the budget restated, the reader of the harness's `finesub` output and the fixture
of the wide cells of palr(256,7) from which the GPU tier draws its frames."""
import os

import numpy as np

FINE_CELLS, QUAD, WINDOW, WIDE_LIST, FINE_IDS, TAG = 32 ** 3, 4, 6, 16, 512, 0x8000
LEAN_TAB_BYTES = 160 * 1024 - 8 * 1024
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fine_sub_palr256_7.npz")


def fine_sub_bytes(n_win, n_wide):
    """quads, their norms and pairs (16 + 16 + 8 bytes a window), a u16 per cell, a row of eight u16 per wide cell"""
    return n_win * 40 + FINE_CELLS * 2 + n_wide * 16


def fine_sub_image_bytes(n_win, n_wide):
    return n_win * WINDOW * 4 + n_wide * (WIDE_LIST * 4 + 16) + FINE_CELLS * 2


def fine_sub_fits(n_win, n_wide):
    return n_wide <= FINE_IDS and fine_sub_bytes(n_win, n_wide) + 16 * 19 * 4 <= LEAN_TAB_BYTES and fine_sub_image_bytes(n_win, n_wide) <= LEAN_TAB_BYTES


def fine_sub_level(f):
    """ordered_fine.h, restated: the two-level table at key level 1, where it and the thresholds fit; 0: today's kernel"""
    if not f["present"] or f["keys"] != 1 or f["cap"] < 1 or f["n_wide"] > FINE_IDS:
        return 0
    return min(f["cap"], 2) if fine_sub_bytes(f["n_win"], f["n_wide"]) + f["thr_bytes"] <= LEAN_TAB_BYTES else 0


def cell_of(rgb):
    rgb = np.asarray(rgb, np.int64)
    return (rgb[..., 0] >> 3) | ((rgb[..., 1] >> 3) << 5) | ((rgb[..., 2] >> 3) << 10)


def sub_of(rgb):
    rgb = np.asarray(rgb, np.int64)
    return ((rgb[..., 0] >> 2) & 1) | (((rgb[..., 1] >> 2) & 1) << 1) | (((rgb[..., 2] >> 2) & 1) << 2)


def colours(cell, sub=None):
    """the 512 colours of a cell, or the 64 of one of its sub-cells, [n, 3]"""
    if sub is None:
        i = np.arange(512)
        return np.stack([(cell & 31) * 8 + (i & 7), ((cell >> 5) & 31) * 8 + ((i >> 3) & 7), (cell >> 10) * 8 + (i >> 6)], -1)
    i = np.arange(64)
    return np.stack([(cell & 31) * 8 + (sub & 1) * 4 + (i & 3), ((cell >> 5) & 31) * 8 + ((sub >> 1) & 1) * 4 + ((i >> 2) & 3),
                     (cell >> 10) * 8 + (sub >> 2) * 4 + (i >> 4)], -1)


def sets(pal, x):
    """N and T of the colours x [n, 3] by brute force over the whole palette: the entries nearest to some colour; everything up to the
    second smallest distance (with multiplicity) of some colour"""
    pal = np.asarray(pal, np.int64).reshape(-1, 3)
    d = ((x[:, None, :] - pal[None, :, :]) ** 2).sum(-1)
    ds = np.sort(d, axis=1)
    return set(np.nonzero((d == ds[:, :1]).any(0))[0].tolist()), set(np.nonzero((d <= ds[:, 1:2]).any(0))[0].tolist())


def read_table(raw):
    """the file `finesub` writes"""
    ok, n_win, n_wide, n_still, words = (int(v) for v in np.frombuffer(raw, "<i4", 5))
    t = dict(ok=ok, n_win=n_win, n_wide=n_wide, n_still=n_still, words=words)
    if not ok:
        return t
    at = 20
    for name, dt, n in (("off", "<u2", FINE_CELLS), ("rows", "<u2", n_wide * 8), ("win_idx", "<u2", n_win * WINDOW), ("wide_cell", "<u2", n_wide),
                        ("sub_wide", "<u2", n_still), ("wide_idx", "<u2", n_wide * WIDE_LIST), ("quad", "<u4", n_win * QUAD),
                        ("pair", "<u4", n_win * (WINDOW - QUAD)), ("wide", "<u4", n_wide * WIDE_LIST), ("image", "<u4", words)):
        t[name] = np.frombuffer(raw, dt, n, at).astype(np.int64)
        at += n * int(dt[2])
    assert at == len(raw)
    return t


def wide_only_colours(n, seed):
    """n colours of the wide cells of palr(256,7), from the fixture: every sub-cell of every wide cell first (the still-wide ones among
    them), then seeded draws from the same cells; shuffled"""
    fx = np.load(FIXTURE)
    cells = fx["wide_cell"].astype(np.int64)
    rs = np.random.RandomState(seed)
    cell = np.concatenate([np.repeat(cells, 8), cells[rs.randint(0, len(cells), max(0, n - 8 * len(cells)))]])
    sub = np.concatenate([np.tile(np.arange(8), len(cells)), rs.randint(0, 8, len(cell) - 8 * len(cells))])
    lo = rs.randint(0, 4, (len(cell), 3))
    rgb = np.stack([(cell & 31) * 8 + (sub & 1) * 4 + lo[:, 0], ((cell >> 5) & 31) * 8 + ((sub >> 1) & 1) * 4 + lo[:, 1],
                    (cell >> 10) * 8 + (sub >> 2) * 4 + lo[:, 2]], -1)
    assert len(rgb) == n, "too few pixels for every sub-cell of every wide cell"
    return rgb[rs.permutation(n)].astype(np.uint8)
