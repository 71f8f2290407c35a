"""GPU tier of the Oklab colour metric (include/ditherpie_hip_metric.h): dp_metric_lab_u8 over all 2^24 colours against the
pin; the top-2 table, exhaustively, against dp_metric_top2_host; ordered output against the numpy statement
tests/metric_ref.py; pattern dithering and dot diffusion on a metric palette against tests/pattern_ref.py / dotdiff_ref.py
through the statement's adapter; the refusals of every entry point that would search a metric palette in RGB; and
ImageDitherer(metric="oklab") end to end."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import dotdiff_ref as dr
import metric_ref as mr
import pattern_ref as pr

pytestmark = pytest.mark.gpu

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
MODE_NEAREST, MODE_MATRIX = 0, 1
SHAPES = [
    (3, 17, 33), (1, 1, 7), (2, 67, 129),
    (3, 4, 7),                                                          # several frames of 84 bytes: the 12-byte dword path; a lane's four pixels straddle a row
    (2, 8, 3),                                                          # w < 4: a lane's four pixels span two rows, 72-byte frames
    (1, 12, 1),                                                         # a lane spans four rows; every matrix is wider than the image
]
ADAPTER = mr.NearestAdapter()


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend, dithering_lib
    yield backend, dithering_lib
    dithering_lib.drop_device_caches()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def palette_of(k, seed=0):
    pal = np.random.RandomState(400 + k + seed).randint(0, 256, (k, 3)).astype(np.float32)
    if k == 5:
        pal[3] = pal[1]                                                  # a duplicate: the lowest index wins, second is the duplicate
    return pal


def index_colours(k):
    """out_colors that encode the chosen index in all three bytes."""
    i = np.arange(k)
    return np.stack([i, i ^ 0x55, 255 - i], axis=1).astype(np.uint8)


def all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], axis=1).astype(np.uint8)


@pytest.fixture(scope="module")
def cube():
    """All 2^24 colours in the order r | g<<8 | b<<16 with their host (L, a, b), computed once."""
    from dither_pie_amd import backend
    rgb = all_colours()
    return rgb, backend.metric_lab_host(rgb)


def matrices(dl):
    m = {s: dl.DitherUtils.get_threshold_matrix(dl.DitherMode.BAYER, s) for s in ("2x2", "4x4", "8x8")}
    m["3x5"] = np.array([[0.0, 0.5, 1.0, 0.25, 0.5], [1.0, 0.0, 0.5, 0.5, 0.75], [0.5, 1.0, 0.0, 0.0, 1.0]], np.float32)
    return m


# ---------------------------------------------------------------------------------------------------- (L, a, b) and the table
def test_lab_of_all_colours(gpu, cube):
    import torch
    be, _ = gpu
    rgb, lab_host = cube
    got = be.metric_lab(torch.from_numpy(rgb).cuda()).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (1 << 24, 3)
    assert hashlib.sha256(got.astype("<i4").tobytes()).hexdigest()[:16] == "fe5bcca474e0af41"
    assert np.array_equal(got, lab_host)


@pytest.mark.parametrize("k", [16, 5, 256])
def test_table_exhaustively_against_the_host_statement(gpu, cube, k):
    """The identity colours as one frame with index-encoding out_colors: DP_MODE_NEAREST gives nearest; DP_MODE_MATRIX with a
    1 x 1 matrix of 0.0 gives second wherever d0 > 0 (f > 0 > t) and nearest where d0 = 0 (f = 0 <= t)."""
    import torch
    be, _ = gpu
    rgb, lab = cube
    side = 4096
    if k == 256:                                                        # a seeded sample of 2^20 colours
        pick = np.random.RandomState(5).randint(0, 1 << 24, 1 << 20)
        rgb, lab, side = rgb[pick], lab[pick], 1024
    pal = palette_of(k)
    w0, w1 = be.metric_top2_host(rgb, pal)
    pal_lab = be.metric_lab_host(pal.astype(np.uint8))
    d0 = ((lab.astype(np.int64) - pal_lab[w0]) ** 2).sum(-1)
    if k != 256:
        assert (d0 == 0).sum() >= len(np.unique(pal, axis=0))           # the palette's own colours are among them
    P = be.Palette(pal, index_colours(k), metric="oklab")
    frame = torch.from_numpy(rgb.reshape(side, side, 3)).cuda()
    near = be.ordered(frame, P, MODE_NEAREST).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(near, index_colours(k)[w0])
    zero = be.Thresholds.from_matrix(np.zeros((1, 1), np.float32))
    sec = be.ordered(frame, P, MODE_MATRIX, thr=zero).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(sec, index_colours(k)[np.where(d0 > 0, w1, w0)])
    del P


# ---------------------------------------------------------------------------------------------------- ordered output
@pytest.mark.parametrize("k", [1, 2, 5, 16, 256])
def test_ordered_matches_the_statement(gpu, k):
    import torch
    be, dl = gpu
    pal, outc = palette_of(k), np.random.RandomState(k).randint(0, 256, (k, 3)).astype(np.uint8)
    P = be.Palette(pal, outc, metric="oklab")                           # the lazy build: the first call makes the table
    mats = matrices(dl)
    assert any(n > 1 and 3 * h * w % 4 == 0 for n, h, w in SHAPES) and any(n > 1 and 3 * h * w % 4 for n, h, w in SHAPES)   # dword and byte path
    assert any(n > 1 and 1 < w < 4 for n, h, w in SHAPES) and any(w == 1 and h > 8 for n, h, w in SHAPES)
    for n, h, w in SHAPES:
        frames = np.random.RandomState(10 * k + h).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        frames[0].reshape(-1, 3)[:k] = pal.astype(np.uint8)[:h * w]     # colours equal to palette entries: d0 = 0
        dev = torch.from_numpy(frames).cuda()
        got = be.ordered(dev, P, MODE_NEAREST).cpu().numpy()
        assert np.array_equal(got, mr.ordered_u8(frames, pal, outc)), (k, n, h, w, "nearest")
        for name, m in mats.items():
            T = be.Thresholds.from_matrix(m)
            for y0, x0 in ((0, 0), (5, 3)):
                want = mr.ordered_u8(frames, pal, outc, m, y0, x0)
                got = be.ordered(dev, P, MODE_MATRIX, thr=T, y0=y0, x0=x0).cpu().numpy()
                bad = np.argwhere((got != want).any(axis=-1))
                assert not len(bad), (k, n, h, w, name, y0, x0, len(bad), bad[:4].tolist())
            inplace = dev.clone()
            assert be.ordered(inplace, P, MODE_MATRIX, thr=T, y0=5, x0=3, out=inplace).data_ptr() == inplace.data_ptr()
            assert np.array_equal(inplace.cpu().numpy(), want), (k, n, h, w, name, "in place")
    del P


def test_prepare_first_and_two_palettes_alive(gpu):
    import torch
    be, dl = gpu
    frames = np.random.RandomState(77).randint(0, 256, (2, 19, 35, 3)).astype(np.uint8)
    dev = torch.from_numpy(frames).cuda()
    m = matrices(dl)["4x4"]
    T = be.Thresholds.from_matrix(m)
    pa, pb = palette_of(16, 1), palette_of(16, 2)
    oa, ob = pa.astype(np.uint8), pb.astype(np.uint8)
    A = be.Palette(pa, oa, metric="oklab")
    B = be.Palette(pb, ob, metric="oklab")
    assert A.metric == B.metric == "oklab" and A._accel_done
    assert A.metric_prepare() == (2 << 24) + 5 * 1024 == A.metric_prepare()          # prepare first, idempotent
    wa, wb = mr.ordered_u8(frames, pa, oa, m, 2, 1), mr.ordered_u8(frames, pb, ob, m, 2, 1)
    assert not np.array_equal(wa, wb)
    for _ in range(2):                                                  # B builds lazily while A's table is alive; neither disturbs the other
        assert np.array_equal(be.ordered(dev, A, MODE_MATRIX, thr=T, y0=2, x0=1).cpu().numpy(), wa)
        assert np.array_equal(be.ordered(dev, B, MODE_MATRIX, thr=T, y0=2, x0=1).cpu().numpy(), wb)
    with pytest.raises(ValueError, match="gradient noise"):
        be.ordered(dev, A, be.MODE_IGN)
    with pytest.raises(ValueError, match="metric"):
        be.Palette(pa, oa).metric_prepare()
    A.build_accel()                                                      # returns at once: a metric palette has no accelerator
    pe = C.c_int(-1)
    from dither_pie_amd import _lib
    assert _lib.load().dp_palette_build_accel(A._h) == DP_OK and _lib.load().dp_palette_accel_info(A._h, C.byref(pe), None) == DP_OK
    assert pe.value == 0
    # metric 0 through dp_palette_create_metric is dp_palette_create: the RGB path, the oracle's pixels
    h = C.c_void_p()
    assert _lib.load().dp_palette_create_metric(pa.ctypes.data, oa.ctypes.data, 16, 0, C.byref(h)) == DP_OK
    assert _lib.load().dp_palette_metric(h) == 0 and _lib.load().dp_metric_table_bytes(h) == 0
    _lib.load().dp_palette_destroy(h)


# ---------------------------------------------------------------------------------------------------- pattern, dot diffusion
@pytest.mark.parametrize("k", [16, 256])
def test_pattern_and_dot_diffusion_use_the_metric(gpu, orc, k):
    import torch
    be, _ = gpu
    pal, outc = palette_of(k, 3), np.random.RandomState(30 + k).randint(0, 256, (k, 3)).astype(np.uint8)
    frames = np.random.RandomState(31 + k).randint(0, 256, (2, 19, 35, 3)).astype(np.uint8)
    dev = torch.from_numpy(frames).cuda()
    P = be.Palette(pal, outc, metric="oklab")
    from dither_pie_amd import _lib
    assert _lib.load().dp_pattern_table_bytes(P._h) == (1 << 24) + 3 * 1024      # keeps its value
    differs = 0
    for m in (2, 4, 8):
        want = pr.pattern_frames(ADAPTER, frames, pal, outc, None, m, 128, y0=1, x0=2)
        got = be.pattern(dev, P, m, 128, y0=1, x0=2).cpu().numpy()
        assert np.array_equal(got, want), (k, m)
        differs += int((want != pr.pattern_frames(orc, frames, pal, outc, None, m, 128, y0=1, x0=2)).any(-1).sum())
    assert differs > 0                                                   # ... and that is not what the RGB search gives
    four = pr.bayer_rank(4)                                              # a 4 x 4 class matrix (a permutation of 0 .. 15)
    for classes in (dr.KNUTH, four):
        want = dr.dotdiff_frames(ADAPTER, frames, pal, outc, None, classes, 256)
        got = be.dotdiff(dev, P, classes, 256).cpu().numpy()
        assert np.array_equal(got, want), (k, classes.shape)
    # the ordered path of the same palette still answers from the top-2 table
    assert np.array_equal(be.ordered(dev, P, MODE_NEAREST).cpu().numpy(), mr.ordered_u8(frames, pal, outc))
    del P


# ---------------------------------------------------------------------------------------------------- refusals
def test_rgb_entry_points_refuse_a_metric_palette(gpu):
    """Silently falling back to RGB is what the feature must rule out: each call returns the unsupported status, names
    itself and leaves its output buffer untouched."""
    import torch
    from dither_pie_amd import _lib
    be, _ = gpu
    L = _lib.load()
    n, h, w = 2, 9, 13
    frames = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (n, h, w, 3)).astype(np.uint8)).cuda()
    out = torch.full_like(frames, 0xA5)
    sets = torch.full((n * h * w,), 0x5A5A, dtype=torch.int16, device="cuda")
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    pal = palette_of(16, 4)
    P = be.Palette(pal, pal.astype(np.uint8), metric="oklab")
    dx, dy, wq = np.array([1], np.int32), np.array([0], np.int32), np.array([0.5], np.float32)
    ht, wl = be.HalftoneParams(), be.WaveletParams()
    i, o, p, s, wp, wb = frames.data_ptr(), out.data_ptr(), P._h, be._stream(), ws.data_ptr(), ws.numel()
    calls = {
        "dp_ordered_u8": lambda: L.dp_ordered_u8(i, o, n, h, w, 0, 0, p, MODE_NEAREST, None, 1.0, 0, wp, wb, s),
        "dp_error_diffusion_u8": lambda: L.dp_error_diffusion_u8(i, o, n, h, w, p, dx.ctypes.data, dy.ctypes.data, wq.ctypes.data, 1, 0, wp, wb, s),
        "dp_error_diffusion_numba_u8": lambda: L.dp_error_diffusion_numba_u8(i, o, n, h, w, p, dx.ctypes.data, dy.ctypes.data, wq.ctypes.data,
                                                                             16.0, 1, 0, wp, wb, s),
        "dp_hybrid_numba_u8": lambda: L.dp_hybrid_numba_u8(i, o, n, h, w, p, 1.0, 0.2, wp, wb, s),
        "dp_riemersma_u8": lambda: L.dp_riemersma_u8(i, o, n, h, w, p, s),
        "dp_halftone_u8": lambda: L.dp_halftone_u8(i, o, n, h, w, p, C.addressof(ht), wp, wb, s),
        "dp_wavelet_u8": lambda: L.dp_wavelet_u8(i, o, n, h, w, p, C.addressof(wl), wp, wb, s),
        "dp_variable_diffusion_u8": lambda: L.dp_variable_diffusion_u8(i, o, n, h, w, p, 1, 0.0, 0.0, 0, None, None, wp, wb, s),
        "dp_variance_gate_u8": lambda: L.dp_variance_gate_u8(i, o, n, h, w, p, 300.0, 1, wp, wb, s),
        "dp_cells_u8": lambda: L.dp_cells_u8(i, o, sets.data_ptr(), n, h, w, p, 8, 8, 2, 0, None, 0, 4, 64, s),
    }
    for name, call in calls.items():
        rc = call()
        torch.cuda.synchronize()
        msg = L.dp_last_error()
        assert rc == DP_EUNSUPPORTED and name.encode() in msg and b"metric" in msg, (name, rc, msg)
    assert bool((out == 0xA5).all()) and bool((sets == 0x5A5A).all()) and not bool(ws.any())
    for fn in (lambda: be.riemersma(frames, P), lambda: be.error_diffusion(frames, P, [(1, 0, 7)], 16)):
        with pytest.raises(be.DitherPieError, match="metric"):
            fn()
    del P


# ---------------------------------------------------------------------------------------------------- ImageDitherer
def test_image_ditherer_end_to_end(gpu):
    import torch
    from PIL import Image
    be, dl = gpu
    pal_list = [tuple(int(v) for v in c) for c in palette_of(16, 6).astype(np.uint8)]
    pal = np.array(pal_list, np.float32)
    outc = pal.astype(np.uint8)
    img = np.random.RandomState(40).randint(0, 256, (17, 33, 3)).astype(np.uint8)      # a 33 x 17 image
    pil = Image.fromarray(img, "RGB")
    bayer4 = dl.DitherUtils.get_threshold_matrix(dl.DitherMode.BAYER, "4x4")
    pat = dl.PatternDitherStrategy("4x4", 0.5)
    wants = {
        dl.DitherMode.BAYER: mr.ordered_u8(img, pal, outc, bayer4),
        dl.DitherMode.NONE: mr.ordered_u8(img, pal, outc),
        pat: pr.pattern_u8(ADAPTER, img, pal, outc, None, 4, 128),
    }
    for mode, want in wants.items():
        d = dl.ImageDitherer(num_colors=16, dither_mode=mode, palette=pal_list, metric="oklab")
        got = np.asarray(d.apply_dithering(pil))
        assert got.shape == (17, 33, 3) and np.array_equal(got, want), mode
        rgb_out = np.asarray(dl.ImageDitherer(num_colors=16, dither_mode=mode, palette=pal_list).apply_dithering(pil))
        assert not np.array_equal(rgb_out, want), mode                   # the two metrics have palettes of their own in the cache
    d = dl.ImageDitherer(num_colors=16, dither_mode=dl.DitherMode.BAYER, palette=pal_list, metric="oklab").prepare()
    want = wants[dl.DitherMode.BAYER]
    dev = torch.from_numpy(img).cuda()
    planes, colours = d.apply_dithering_frames_indexed(dev)              # the indexed path
    assert np.array_equal(colours, outc) and np.array_equal(colours[planes.cpu().numpy().astype(np.int64)], want)
    assert np.array_equal(np.asarray(d.apply_dithering_indexed(pil).convert("RGB")), want)
    top = d.apply_dithering_frames(dev[:7].contiguous(), y0=0, x0=0).cpu().numpy()     # two row bands reassemble to the whole image
    bottom = d.apply_dithering_frames(dev[7:].contiguous(), y0=7, x0=0).cpu().numpy()
    assert np.array_equal(np.concatenate([top, bottom]), want)
    for mode in (dl.DitherMode.ERROR_DIFFUSION, dl.DitherMode.INTERLEAVED_GRADIENT_NOISE, dl.CellPaletteDitherStrategy()):
        with pytest.raises(ValueError, match="oklab"):
            dl.ImageDitherer(num_colors=16, dither_mode=mode, palette=pal_list, metric="oklab").apply_dithering(pil)
