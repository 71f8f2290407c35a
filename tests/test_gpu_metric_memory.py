"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_metric.h on the guarded arena
(tests/arena.py), as tests/test_gpu_pattern_memory.py is for the pattern header: the buffers the library sees lie inside one
arena, have exactly their size and sit at odd addresses (lab_dev at the 4-byte alignment the header asks for, and no better);
whatever the output held before -- zeros, 0xFF, noise -- the result is that of tests/metric_ref.py; guards of >= 1 MiB stay
intact; inputs are unchanged; a refused call launches nothing and leaves every buffer as it was.  dp_metric_prepare takes no
buffer of the caller's: it is run with the arena live (its table is the library's own allocation) and must leave guards and
regions alone, and the call that follows must give the pixels of the lazy path.  tests/test_metric_cpu.py checks COVERAGE
against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import metric_ref as mr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_metric_ordered_u8": ["test_metric_ordered_on_the_arena"],
    "dp_metric_prepare": ["test_metric_ordered_on_the_arena"],
    "dp_metric_lab_u8": ["test_metric_lab_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
MODE_NEAREST, MODE_MATRIX, MODE_IGN = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(93))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, frames, h, w, colours, threshold matrix shape (None: nearest only), residues of in / out (odd, and different), prepare first
@pytest.mark.parametrize("case, n, h, w, k, tshape, r_in, r_out, prepare", [
    (0, 3, 17, 33, 16, (4, 4), 1, 7, False),
    (1, 2, 67, 129, 256, (3, 5), 3, 5, True),
    (2, 1, 1, 7, 5, None, 15, 9, True),
    (3, 2, 3, 5, 2, (8, 8), 5, 11, False),
    (4, 2, 16, 16, 1, (2, 2), 4, 8, False),       # frames that are whole dwords at dword addresses: the 12-byte path
])
def test_metric_ordered_on_the_arena(gpu, case, n, h, w, k, tshape, r_in, r_out, prepare):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(60 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    pal = rs.randint(0, 256, (k, 3)).astype(np.float32)
    outc = rs.randint(0, 256, (k, 3)).astype(np.uint8)
    thr = None if tshape is None else rs.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), tshape).astype(np.float32)
    y0, x0 = case, 2 * case + 1
    want = mr.ordered_u8(frames, pal, outc, thr, y0, x0)
    P = be.Palette(pal, outc, metric="oklab")
    T = None if thr is None else be.Thresholds.from_matrix(thr)
    mode = MODE_NEAREST if thr is None else MODE_MATRIX
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g)]), "cuda", 80 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes
    A.put("in", frames)
    A.carve("out", frames.nbytes, r_out, g)
    assert A.ptr("in") % 16 == r_in and A.ptr("out") % 16 == r_out
    st = be._stream()
    if prepare:
        A.fill("out", FILLS[0])
        assert L.dp_metric_prepare(P._h) == DP_OK, L.dp_last_error()
        assert L.dp_metric_prepare(P._h) == DP_OK                       # idempotent
        torch.cuda.synchronize()
        A.check()
        A.unchanged("in")
        A.unchanged("out")
    assert L.dp_metric_table_bytes(P._h) == (2 << 24) + 5 * 1024 and L.dp_palette_metric(P._h) == 1
    for i, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + i)
        A.fill("out", fill)
        rc = L.dp_metric_ordered_u8(A.ptr("in"), A.ptr("out"), n, h, w, y0, x0, P._h, mode, T._h if T else None, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("out").reshape(n, h, w, 3), want), (case, fill)
        A.check()
        A.unchanged("in")

    # refusals launch nothing: every buffer keeps what it holds
    A.put("out", A.get("out").copy())
    rgb_pal = be.Palette(pal, outc)
    for kw, code in ((dict(i=None), DP_EINVAL), (dict(o=None), DP_EINVAL), (dict(h=0), DP_EINVAL), (dict(w=-1), DP_EINVAL),
                     (dict(y0=-1), DP_EINVAL), (dict(x0=-3), DP_EINVAL), (dict(pal=None), DP_EINVAL), (dict(n=-1), DP_EINVAL),
                     (dict(mode=3), DP_EINVAL), (dict(mode=-1), DP_EINVAL), (dict(mode=MODE_MATRIX, thr=None), DP_EINVAL),
                     (dict(mode=MODE_IGN), DP_EUNSUPPORTED), (dict(pal=rgb_pal._h), DP_EINVAL)):
        v = dict(i=A.ptr("in"), o=A.ptr("out"), n=n, h=h, w=w, y0=0, x0=0, pal=P._h, mode=mode, thr=T._h if T else None)
        v.update(kw)
        rc = L.dp_metric_ordered_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["y0"], v["x0"], v["pal"], v["mode"], v["thr"], st)
        torch.cuda.synchronize()
        assert rc == code and b"dp_metric_ordered_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_metric_ordered_u8(A.ptr("in"), A.ptr("out"), 0, h, w, 0, 0, P._h, mode, T._h if T else None, st) == DP_OK   # n_frames = 0: a no-op
    assert L.dp_metric_prepare(rgb_pal._h) == DP_EINVAL and b"dp_metric_prepare" in L.dp_last_error()
    assert L.dp_metric_table_bytes(rgb_pal._h) == 0 and L.dp_palette_metric(rgb_pal._h) == 0
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("out")
    A.check()
    del A


@pytest.mark.parametrize("case, n_px, r_in, r_out", [(0, 1, 1, 4), (1, 257, 7, 12), (2, 5000, 9, 4)])
def test_metric_lab_on_the_arena(gpu, case, n_px, r_in, r_out):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rgb = np.random.RandomState(70 + case).randint(0, 256, (n_px, 3)).astype(np.uint8)
    want = mr.lab(rgb)
    A = ar.Arena(ar.capacity_for([(rgb.nbytes, g), (12 * n_px, g)]), "cuda", 90 + case)
    A.carve("in", rgb.nbytes, r_in, g)
    A.put("in", rgb)
    A.carve("lab", 12 * n_px, r_out, g)                                 # exactly 3 int32 per pixel, 4-byte aligned and no better
    assert A.ptr("in") % 2 == 1 and A.ptr("lab") % 16 == r_out
    st = be._stream()
    for i, fill in enumerate(FILLS):
        A.reseed(950 + 10 * case + i)
        A.fill("lab", fill)
        rc = L.dp_metric_lab_u8(A.ptr("in"), A.ptr("lab"), n_px, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("lab", np.int32).reshape(n_px, 3), want), (case, fill)
        A.check()
        A.unchanged("in")
    A.put("lab", A.get("lab").copy())
    for kw in (dict(i=None), dict(o=None), dict(n=-1), dict(n=1 << 31), dict(o=A.ptr("lab") + 2), dict(o=A.ptr("lab") + 1)):
        v = dict(i=A.ptr("in"), o=A.ptr("lab"), n=n_px)
        v.update(kw)
        rc = L.dp_metric_lab_u8(v["i"], v["o"], v["n"], st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_metric_lab_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_metric_lab_u8(A.ptr("in"), A.ptr("lab"), 0, st) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("lab")
    A.check()
    del A
