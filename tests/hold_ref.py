"""The temporal hold in numpy: the normative statement of include/ditherpie_hip_hold.h (host: csrc/host_logic.h hold_apply; device:
csrc/hold.hip), and the inputs the hold tests share.

hold(src, planes, state, cell, tol, share256) -> (out, refreshed, state'):
  src [N,H,W,3] uint8, planes [N,H,W] uint8; state = None (the first frame of a stream) or (anchor [H,W,3], held [H,W]).
  The frame is cut into cell x cell cells from the top-left corner, clipped at the right and bottom edges.  Frame by frame:
  without state every pixel refreshes; otherwise a pixel is changed iff max_c |src - anchor| > tol, and a cell refreshes iff
  changed_count > 0 and changed_count * 256 >= share256 * cell_px.  Pixels of refreshing cells take anchor = src, held = planes;
  out[f] = held, refreshed[f] = the pixels refreshed (int64).  Nothing is modified in place."""
import numpy as np

CELLS = (1, 2, 4, 8, 16)

# (N, H, W, cell, tol, share256): the cases of the issue, then one each for cell 2 and cell 8 at share256 = 128
CASES = [(5, 17, 19, 16, 3, 0), (4, 1, 1, 1, 0, 0), (6, 9, 67, 4, 2, 64), (5, 33, 5, 8, 0, 256), (3, 16, 16, 16, 1, 1),
         (4, 7, 10, 2, 5, 128), (4, 20, 27, 8, 6, 128)]


def check_settings(cell, tol, share256):
    if cell not in CELLS:
        raise ValueError(f"cell must be one of {CELLS}, not {cell!r}")
    if not 0 <= int(tol) <= 255:
        raise ValueError("tol must be in 0 ... 255")
    if not 0 <= int(share256) <= 256:
        raise ValueError("share256 must be in 0 ... 256")


def cell_sums(a, cell):
    """[H,W] -> the sums over the (clipped) cells, [ceil(H / cell), ceil(W / cell)] int64"""
    h, w = a.shape
    rows = np.add.reduceat(a.astype(np.int64), np.arange(0, h, cell), axis=0)
    return np.add.reduceat(rows, np.arange(0, w, cell), axis=1)


def refresh_mask(src_f, anchor, cell, tol, share256):
    """The pixels frame src_f refreshes against `anchor`, [H,W] bool."""
    h, w, _ = src_f.shape
    diff = np.abs(src_f.astype(np.int16) - anchor.astype(np.int16)).max(axis=-1)
    changed = cell_sums(diff > tol, cell)
    cell_px = cell_sums(np.ones((h, w), np.int64), cell)
    cells = (changed > 0) & (changed * 256 >= share256 * cell_px)
    return np.repeat(np.repeat(cells, cell, axis=0), cell, axis=1)[:h, :w]


def hold(src, planes, state, cell, tol, share256):
    src, planes = np.asarray(src), np.asarray(planes)
    assert src.dtype == np.uint8 and planes.dtype == np.uint8 and src.ndim == 4 and src.shape[-1] == 3 and planes.shape == src.shape[:3]
    check_settings(cell, tol, share256)
    n, h, w, _ = src.shape
    anchor, held = (None, None) if state is None else (state[0].copy(), state[1].copy())
    out = np.empty((n, h, w), np.uint8)
    refreshed = np.zeros(n, np.int64)
    for f in range(n):
        if anchor is None:
            anchor, held = src[f].copy(), planes[f].copy()
            refreshed[f] = h * w
        else:
            m = refresh_mask(src[f], anchor, cell, tol, share256)
            anchor[m] = src[f][m]
            held[m] = planes[f][m]
            refreshed[f] = int(m.sum())
        out[f] = held
    return out, refreshed, (None if anchor is None else (anchor, held))


def block_extent(size, cell):
    """The block of clip(): from 0 up to half the size rounded down to whole cells, one cell at least, the size at most."""
    return min(size, max(cell, (size // 2) // cell * cell))


def clip(n, h, w, cell, tol, seed, colours=16):
    """A fixed base image plus noise of at most tol // 2 per channel (so two frames of the base differ by at most tol wherever they
    are compared), and a block at the top-left corner -- whole cells where the frame has them -- that is replaced (+128 mod 256)
    from frame n // 2 on.  The planes are independent random indices per frame: the worst case for flicker.
    -> src [n,h,w,3] uint8, planes [n,h,w] uint8"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3)).astype(np.int16)
    moved = base.copy()
    bh, bw = block_extent(h, cell), block_extent(w, cell)
    moved[:bh, :bw] = (moved[:bh, :bw] + 128) % 256
    amp = tol // 2
    src = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        noise = rng.integers(-amp, amp + 1, (h, w, 3))
        src[f] = np.clip((moved if f >= n // 2 else base) + noise, 0, 255).astype(np.uint8)
    planes = rng.integers(0, colours, (n, h, w)).astype(np.uint8)
    return src, planes
