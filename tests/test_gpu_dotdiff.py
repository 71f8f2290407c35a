"""GPU tier of dot diffusion: byte equality of dp_dotdiff_u8 (through backend.dotdiff, DotDiffusionDitherStrategy and the
instance hook of ImageDitherer) with the numpy statement tests/dotdiff_ref.py, which goes class by class and knows nothing
of tiles or levels.  The grid: every shape x batch x strength for each palette and class matrix; the shapes end in one of
three tiles each way with ragged edges, so that halos are clipped on every side and meet in the middle; one matrix has reach
exactly 16, the halo of the kernel.  Then the properties that need no reference and the ImageDitherer / video paths."""
import io

import numpy as np
import pytest

import dotdiff_ref as dr

pytestmark = pytest.mark.gpu

T = 64                                                                  # backend.DOTDIFF_TILE (checked below)
SHAPES = [(1, 1), (1, 7), (3, 5), (17, 33), (2 * T + 19, 3 * T + 5)]
STRENGTHS = (0, 77, 256)


def _search(seed, m, want):
    """The first permutation drawn from RandomState(seed) whose reach is `want`, and its draw number."""
    rs = np.random.RandomState(seed)
    for draw in range(2000):
        M = rs.permutation(m * m).reshape(m, m)
        if dr.reach(M) == want:
            return draw, M
    raise AssertionError((seed, m, want))


def bayer4():
    import pattern_ref as pr
    return pr.bayer_rank(4)


MATRICES = {
    "knuth": lambda: dr.KNUTH,
    "bayer4": bayer4,
    "random16": lambda: np.random.RandomState(2033).permutation(256).reshape(16, 16),
    "reach16": lambda: _search(2032, 8, 16)[1],
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend, dithering_lib
    assert backend.DOTDIFF_TILE == T
    yield backend, dithering_lib
    dithering_lib.drop_device_caches()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def palette_of(k):
    """The palette list (RGB triples) of the K cases (those of tests/test_gpu_pattern.py)."""
    from test_gpu_pattern import palette_of as pattern_palette
    return pattern_palette(k)


def frames_of(k, h, w):
    """Three distinct frames: noise, a gradient with noise, dark noise; with the tie pixels for the tie palette."""
    from test_gpu_pattern import frames_of as pattern_frames
    return pattern_frames(k, h, w)


def test_the_searched_matrices_are_what_the_grid_needs():
    assert _search(2032, 8, 16)[0] == 1 and _search(2032, 8, 17)[0] == 767
    assert _search(2040, 16, 16)[0] == 2 and _search(2040, 16, 17)[0] == 84
    assert dr.reach(MATRICES["reach16"]()) == 16 == dr.MAX_REACH and dr.reach(dr.KNUTH) == 14 and dr.reach(bayer4()) == 3
    assert dr.reach(MATRICES["random16"]()) <= 16


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("k", [1, 2, 16, 256])
def test_matches_the_statement_over_the_grid(gpu, orc, k, gamma, name):
    import torch
    be, dl = gpu
    M = MATRICES[name]()
    pal_f32, outc, lut = dl.prepare_palette(palette_of(k), gamma)
    assert pal_f32.shape == (k, 3)
    P = be.Palette(pal_f32, outc, lut)
    for h, w in SHAPES:
        frames = frames_of(k, h, w)
        dev = torch.from_numpy(frames).cuda()
        for s in STRENGTHS:
            want = dr.dotdiff_frames(orc, frames, pal_f32, outc, lut, M, s)
            got3 = be.dotdiff(dev, P, M, s).cpu().numpy()
            got1 = be.dotdiff(dev[:1].clone(), P, M, s).cpu().numpy()
            bad = np.argwhere((got3 != want).any(axis=-1))
            assert not len(bad), (k, gamma, name, h, w, s, len(bad), bad[:4].tolist())
            assert np.array_equal(got1, want[:1]), (k, gamma, name, h, w, s, "N = 1")
    del P


def test_the_reach_16_matrix_of_sixteen(gpu, orc):
    """The 16 x 16 matrix of reach exactly 16 on the multi-tile shape."""
    import torch
    be, dl = gpu
    M = _search(2040, 16, 16)[1]
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(pal_f32, outc, lut)
    frames = frames_of(16, *SHAPES[-1])
    want = dr.dotdiff_frames(orc, frames, pal_f32, outc, lut, M, 256)
    assert np.array_equal(be.dotdiff(torch.from_numpy(frames).cuda(), P, M, 256).cpu().numpy(), want)


def test_a_reach_17_matrix_is_refused_and_the_output_untouched(gpu):
    import torch
    be, dl = gpu
    from dither_pie_amd import _lib
    L = _lib.load()
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(pal_f32, outc, lut)
    frames = torch.from_numpy(frames_of(16, 17, 33)).cuda()
    for seed, m in ((2032, 8), (2040, 16)):
        M = np.ascontiguousarray(_search(seed, m, 17)[1], np.uint8)
        assert be.dotdiff_reach(M) == 17
        out = torch.full_like(frames, 0xA5)
        rc = L.dp_dotdiff_u8(frames.data_ptr(), out.data_ptr(), 3, 17, 33, P._h, M.ctypes.data, m, 256, be._stream())
        torch.cuda.synchronize()
        msg = L.dp_last_error()
        assert rc == 2 and b"dp_dotdiff_u8" in msg and b"reach 17" in msg, (rc, msg)   # DP_EUNSUPPORTED
        assert bool((out == 0xA5).all())
        with pytest.raises(ValueError, match="reach 17"):
            be.dotdiff(frames, P, M, 256, out=out)
        assert bool((out == 0xA5).all())


@pytest.mark.parametrize("gamma", [False, True])
def test_strength_zero_is_no_dither_on_the_device(gpu, gamma):
    import torch
    be, dl = gpu
    frames = torch.from_numpy(frames_of(16, *SHAPES[-1])).cuda()
    for k in (2, 16, 256):
        pal = palette_of(k)
        want = dl.ImageDitherer(dither_mode=dl.DitherMode.NONE, palette=pal, use_gamma=gamma).apply_dithering_frames(frames)
        for matrix in ("knuth", bayer4()):
            got = dl.DotDiffusionDitherStrategy(matrix, 0.0).dither_frames(frames, pal, gamma)
            assert torch.equal(got, want), (k, gamma)


def test_repeatable_batches_and_out_buffers(gpu):
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(pal_f32, outc, lut)
    frames = torch.from_numpy(frames_of(16, *SHAPES[-1])).cuda()
    want = be.dotdiff(frames, P, dr.KNUTH, 256)
    assert torch.equal(be.dotdiff(frames, P, dr.KNUTH, 256), want)       # two calls give the same bytes
    for i in range(3):                                                   # a batch equals its frames one by one
        one = be.dotdiff(frames[i], P, dr.KNUTH, 256)                    # [H,W,3]
        assert one.shape == frames[i].shape and torch.equal(one, want[i]), i
    assert not torch.equal(want[0], want[1])
    buf = torch.full_like(frames, 0xAB)
    got = be.dotdiff(frames, P, dr.KNUTH, 256, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    # out = in is refused, by the wrapper and by the library, and nothing is written
    keep = frames.clone()
    with pytest.raises(ValueError, match="in place"):
        be.dotdiff(frames, P, dr.KNUTH, 256, out=frames)
    from dither_pie_amd import _lib
    L = _lib.load()
    M = np.ascontiguousarray(dr.KNUTH, np.uint8)
    n, h, w, _ = frames.shape
    rc = L.dp_dotdiff_u8(frames.data_ptr(), frames.data_ptr(), n, h, w, P._h, M.ctypes.data, 8, 256, be._stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"dp_dotdiff_u8" in L.dp_last_error() and b"in_dev" in L.dp_last_error()   # DP_EINVAL
    assert torch.equal(frames, keep)
    with pytest.raises(ValueError):
        be.dotdiff(frames, P, dr.KNUTH, 256, out=torch.zeros(5, dtype=torch.uint8, device="cuda"))
    s = dl.DotDiffusionDitherStrategy()
    assert torch.equal(s.dither_frames(frames, palette_of(16)), want)
    planes, colours = s.dither_frames_indexed(frames, palette_of(16))
    assert planes.dtype == torch.uint8 and planes.shape == frames.shape[:3]
    assert np.array_equal(colours[planes.cpu().numpy()], want.cpu().numpy())
    with pytest.raises(ValueError, match="tiled"):
        s._run(frames, P, y0=8)
    # the strategy contract of the reference: float pixels and palette in, float palette rows out
    small = torch.from_numpy(frames_of(16, 17, 33)).cuda()
    px = small[0].cpu().numpy().reshape(-1, 3).astype(np.float32)
    back = s.dither(px, np.array(palette_of(16), np.float32), (17, 33))
    assert back.shape == px.shape
    assert np.array_equal(back.astype(np.uint8).reshape(17, 33, 3), be.dotdiff(small[0], P, dr.KNUTH, 256).cpu().numpy())


@pytest.mark.parametrize("cap", [1, 2, 5])
def test_workgroups_walk_several_tiles(gpu, orc, switches, cap):
    """The experiments library with a capped grid: every workgroup takes several of the nine tiles in turn, which in the
    product only an image of more than 2^20 tiles does (a single column of 2^26 pixels or more)."""
    import torch
    be, dl = gpu
    switches.setenv("DP_DOTDIFF_GRID_CAP", str(cap))
    M = MATRICES["reach16"]()
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), True)
    P = be.Palette(pal_f32, outc, lut)
    frames = frames_of(16, *SHAPES[-1])
    want = dr.dotdiff_frames(orc, frames, pal_f32, outc, lut, M, 256)
    got = be.dotdiff(torch.from_numpy(frames).cuda(), P, M, 256).cpu().numpy()
    bad = np.argwhere((got != want).any(axis=-1))
    assert not len(bad), (cap, len(bad), bad[:4].tolist())
    del P


def test_one_table_serves_both_modes(gpu, orc):
    """A palette first used by dot diffusion and then by pattern dithering, and the other way round."""
    import torch
    import pattern_ref as pr
    be, dl = gpu
    frames = frames_of(16, 17, 33)
    dev = torch.from_numpy(frames).cuda()
    spec = dl.prepare_palette(palette_of(16), True)
    want_dot = dr.dotdiff_frames(orc, frames, *spec, dr.KNUTH, 256)
    want_pat = pr.pattern_frames(orc, frames, *spec, 4, 128)
    A, B, C_ = be.Palette(*spec), be.Palette(*spec), be.Palette(*spec)
    assert np.array_equal(be.dotdiff(dev, A, dr.KNUTH, 256).cpu().numpy(), want_dot)
    assert np.array_equal(be.pattern(dev, A, 4, 128).cpu().numpy(), want_pat)
    assert np.array_equal(be.pattern(dev, B, 4, 128).cpu().numpy(), want_pat)
    assert np.array_equal(be.dotdiff(dev, B, dr.KNUTH, 256).cpu().numpy(), want_dot)
    assert C_.pattern_prepare() == (1 << 24) + 3 * 1024                  # built ahead: serves dot diffusion too
    assert np.array_equal(be.dotdiff(dev, C_, dr.KNUTH, 256).cpu().numpy(), want_dot)


def test_image_ditherer_paths_with_the_instance(gpu, orc):
    import torch
    from PIL import Image
    be, dl = gpu
    from dither_pie_amd import video_processor as vp
    rs = np.random.RandomState(31)
    arr = rs.randint(0, 256, (17, 33, 3)).astype(np.uint8)              # a 33 x 17 image
    arr[:, :, 1] = np.linspace(0, 255, 33).astype(np.uint8)[None, :]
    img = Image.fromarray(arr, "RGB")
    for gamma in (False, True):
        pal = palette_of(16)
        s = dl.DotDiffusionDitherStrategy()
        d = dl.ImageDitherer(num_colors=16, dither_mode=s, palette=pal, use_gamma=gamma)
        pal_f32, outc, lut = dl.prepare_palette(pal, gamma)
        want = dr.dotdiff_u8(orc, arr, pal_f32, outc, lut, dr.KNUTH, 256)
        got = d.apply_dithering(img)
        assert got.mode == "RGB" and got.size == (33, 17) and np.array_equal(np.asarray(got), want), gamma
        p_img = d.apply_dithering_indexed(img)
        assert p_img.mode == "P" and np.array_equal(np.asarray(p_img.convert("RGB")), want), gamma
        png = d.apply_dithering_png(img)
        dec = Image.open(io.BytesIO(png))
        assert dec.mode == "P" and np.array_equal(np.asarray(dec.convert("RGB")), want), gamma
        # three frames through the video pipeline's batch functions
        stack = np.stack([arr, arr[::-1].copy(), 255 - arr])
        frames = torch.from_numpy(stack).cuda()
        rgb = vp.process_frames(frames, d)
        assert np.array_equal(rgb.cpu().numpy(), dr.dotdiff_frames(orc, stack, pal_f32, outc, lut, dr.KNUTH, 256)), gamma
        planes, colours = vp.process_frames_indexed(frames, d)
        assert planes.shape == (3, 17, 33) and np.array_equal(colours[planes.cpu().numpy()], rgb.cpu().numpy()), gamma
    assert d.dither_mode is s                                           # the hook stores nothing and replaces nothing
    from dither_pie_amd import sharding
    with pytest.raises(ValueError):                                     # errors cross band edges: no row-band sharding
        sharding.dither_band(d, frames[0, :8].contiguous(), 0)
