"""GPU tier of pattern (Knoll) dithering: byte equality of dp_pattern_u8 (through backend.pattern, PatternDitherStrategy and
the instance hook of ImageDitherer) with the numpy statement tests/pattern_ref.py, whose nearest() is the CPU oracle's
nearest-only search.  The grid: every shape x batch x matrix x strength for each palette; the palettes carry a real nearest
tie, duplicate entries, two distinct colours of equal luminance and a median-cut palette.  Then the properties that need no
reference (strength 0 = NoDitherStrategy, tiles reassemble, stale tables) and the ImageDitherer / video paths."""
import io

import numpy as np
import pytest

import pattern_ref as pr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (3, 5), (17, 33), (67, 129)]                  # none a multiple of m or of a wave
MATRICES = (2, 4, 8)
STRENGTHS = (0, 77, 128, 256)


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


def equal_luminance_pair():
    """Two distinct colours with the same 299 r + 587 g + 114 b, found by search."""
    seen = {}
    rs = np.random.RandomState(12)
    for r, g, b in rs.randint(0, 256, (4000, 3)).tolist():
        lum = 299 * r + 587 * g + 114 * b
        if lum in seen and seen[lum] != (r, g, b):
            return seen[lum], (r, g, b)
        seen[lum] = (r, g, b)
    return None


def palette_of(k):
    """The palette list (RGB triples) of the K cases."""
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    if k == 1:
        return [(37, 150, 201)]
    if k == 2:
        return [(0, 0, 0), (2, 0, 0)]                                   # (1, 0, 0) is a real nearest tie
    if k == 5:
        return [(10, 20, 30), (200, 50, 50), (10, 20, 30), (0, 255, 0), (200, 50, 50)]   # duplicate entries
    if k == 16:
        img = np.random.RandomState(21).randint(0, 256, (24, 24, 3)).astype(np.uint8)
        img[:, :12] //= 3                                                # a dark half: crowded entries
        pal = ColorReducer.reduce_colors(Image.fromarray(img, "RGB"), 16)   # a median-cut palette of a small image
        assert len(pal) == 16
        return [tuple(int(v) for v in c) for c in pal]
    pair = equal_luminance_pair()
    assert pair is not None and pair[0] != pair[1]
    assert 299 * pair[0][0] + 587 * pair[0][1] + 114 * pair[0][2] == 299 * pair[1][0] + 587 * pair[1][1] + 114 * pair[1][2]
    rest = np.random.RandomState(22).randint(0, 256, (254, 3)).tolist()
    return [tuple(c) for c in rest[:100]] + [pair[1]] + [tuple(c) for c in rest[100:]] + [pair[0]]   # the later one first in index


def frames_of(k, h, w):
    """Three distinct frames: noise, a gradient with noise, dark noise; with the tie pixels for the tie palette."""
    rs = np.random.RandomState(1000 * k + 10 * h + w)
    f = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    f[1, ..., 0] = (xx * 255 // max(w - 1, 1)).astype(np.uint8)
    f[1, ..., 1] = (yy * 255 // max(h - 1, 1)).astype(np.uint8)
    f[2] //= 8
    if k == 2:
        f[0] = rs.randint(0, 4, (h, w, 3)).astype(np.uint8)
        f[0, ::2, ::3] = (1, 0, 0)
        f[2, :, ::2] = (1, 0, 0)
    return f


@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("k", [1, 2, 5, 16, 256])
def test_matches_the_statement_over_the_grid(gpu, orc, k, gamma):
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette(palette_of(k), gamma)
    assert pal_f32.shape == (k, 3)
    P = be.Palette(pal_f32, outc, lut)
    for h, w in SHAPES:
        frames = frames_of(k, h, w)
        dev = torch.from_numpy(frames).cuda()
        for m in MATRICES:
            for s in STRENGTHS:
                want = pr.pattern_frames(orc, frames, pal_f32, outc, lut, m, s)
                got3 = be.pattern(dev, P, m, s).cpu().numpy()
                got1 = be.pattern(dev[:1].clone(), P, m, s).cpu().numpy()
                bad = np.argwhere((got3 != want).any(axis=-1))
                assert not len(bad), (k, gamma, h, w, m, s, len(bad), bad[:4].tolist())
                assert np.array_equal(got1, want[:1]), (k, gamma, h, w, m, s, "N = 1")
    del P


def test_the_tie_follows_the_nearest_only_mode(gpu, orc):
    """[(0,0,0), (2,0,0)] and pixels (1,0,0): whichever entry the nearest-only mode picks, every candidate is that one."""
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette([(0, 0, 0), (2, 0, 0)], False)
    P = be.Palette(pal_f32, outc, None)
    img = np.zeros((5, 9, 3), np.uint8)
    img[..., 0] = 1
    dev = torch.from_numpy(img).cuda()
    near = be.ordered(dev, P, be.MODE_NEAREST).cpu().numpy()
    assert np.array_equal(near, orc.ordered_u8(img, pal_f32, outc, None, "none"))
    assert np.array_equal(be.pattern(dev, P, 4, 0).cpu().numpy(), near)
    assert np.array_equal(be.pattern(dev, P, 4, 256).cpu().numpy(), pr.pattern_u8(orc, img, pal_f32, outc, None, 4, 256))


@pytest.mark.parametrize("gamma", [False, True])
def test_strength_zero_is_no_dither_on_the_device(gpu, gamma):
    import torch
    be, dl = gpu
    frames = torch.from_numpy(frames_of(16, 67, 129)).cuda()
    for k in (2, 16, 256):
        pal = palette_of(k)
        want = dl.ImageDitherer(dither_mode=dl.DitherMode.NONE, palette=pal, use_gamma=gamma).apply_dithering_frames(frames)
        for name in ("2x2", "4x4", "8x8"):
            got = dl.PatternDitherStrategy(name, 0.0).dither_frames(frames, pal, gamma)
            assert torch.equal(got, want), (k, gamma, name)


def test_bands_and_tiles_reassemble(gpu):
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(pal_f32, outc, lut)
    frames = torch.from_numpy(frames_of(16, 67, 129)).cuda()
    for m, s in ((2, 256), (4, 128), (8, 77)):
        whole = be.pattern(frames, P, m, s)
        out = torch.zeros_like(whole)
        for y_lo, y_hi in ((0, 3), (3, 13), (13, 50), (50, 67)):         # offsets that are no multiples of m
            for x_lo, x_hi in ((0, 5), (5, 6), (6, 75), (75, 129)):
                out[:, y_lo:y_hi, x_lo:x_hi] = be.pattern(frames[:, y_lo:y_hi, x_lo:x_hi].contiguous(), P, m, s, y0=y_lo, x0=x_lo)
        assert torch.equal(out, whole), (m, s)
        assert not torch.equal(be.pattern(frames, P, m, s, y0=1, x0=0), whole)   # the offset does move the pattern
    # the sharded row bands take the strategy instance
    from dither_pie_amd import sharding
    d = dl.ImageDitherer(dither_mode=dl.PatternDitherStrategy("4x4", 0.5), palette=palette_of(16))
    whole = d.apply_dithering_frames(frames[0])
    bands = [sharding.dither_band(d, frames[0, lo:hi].contiguous(), lo) for lo, hi in ((0, 21), (21, 22), (22, 67))]
    assert torch.equal(torch.cat(bands), whole)
    with pytest.raises(ValueError):
        sharding.dither_band(dl.ImageDitherer(dither_mode=dl.HalftoneDitherStrategy(), palette=palette_of(16)), frames[0, :8].contiguous(), 0)


def test_out_buffers_and_three_dimensional_input(gpu):
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette(palette_of(5), False)
    P = be.Palette(pal_f32, outc, lut)
    frames = torch.from_numpy(frames_of(5, 17, 33)).cuda()
    want = be.pattern(frames, P, 4, 128)
    buf = torch.full_like(frames, 0xAB)
    got = be.pattern(frames, P, 4, 128, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    one = be.pattern(frames[1], P, 4, 128)                              # [H,W,3]
    assert one.shape == (17, 33, 3) and torch.equal(one, want[1])
    flat = torch.zeros(frames[2].numel(), dtype=torch.uint8, device="cuda")
    assert torch.equal(be.pattern(frames[2], P, 4, 128, out=flat).view(17, 33, 3), want[2])
    inplace = frames.clone()
    be.pattern(inplace, P, 4, 128, out=inplace)                         # out = in: a lane reads its pixels before it writes
    assert torch.equal(inplace, want)
    with pytest.raises(ValueError):
        be.pattern(frames, P, 4, 128, out=torch.zeros(5, dtype=torch.uint8, device="cuda"))
    s = dl.PatternDitherStrategy("4x4", 0.5)
    assert torch.equal(s.dither_frames(frames, palette_of(5)), want)
    planes, colours = s.dither_frames_indexed(frames, palette_of(5))
    assert planes.dtype == torch.uint8 and planes.shape == (3, 17, 33)
    assert np.array_equal(colours[planes.cpu().numpy()], want.cpu().numpy())
    # the strategy contract of the reference: float pixels and palette in, float palette rows out
    px = frames[0].cpu().numpy().reshape(-1, 3).astype(np.float32)
    back = s.dither(px, np.array(palette_of(5), np.float32), (17, 33))
    assert back.shape == px.shape and np.array_equal(back.astype(np.uint8).reshape(17, 33, 3), want[0].cpu().numpy())


def test_tables_stay_with_their_palettes(gpu, orc):
    """Two palettes used alternately, and a palette destroyed and re-created (its memory may be handed out again)."""
    import torch
    be, dl = gpu
    frames = frames_of(16, 17, 33)
    dev = torch.from_numpy(frames).cuda()
    pals = [dl.prepare_palette(palette_of(16), False), dl.prepare_palette(palette_of(5), False)]
    want = [pr.pattern_frames(orc, frames, p[0], p[1], p[2], 4, 200) for p in pals]
    A, B = be.Palette(*pals[0]), be.Palette(*pals[1])
    for _ in range(3):
        assert np.array_equal(be.pattern(dev, A, 4, 200).cpu().numpy(), want[0])
        assert np.array_equal(be.pattern(dev, B, 4, 200).cpu().numpy(), want[1])
    del A
    torch.cuda.synchronize()
    C_ = be.Palette(*pals[1])                                           # where A's table was, B's colours now
    A2 = be.Palette(*pals[0])
    assert np.array_equal(be.pattern(dev, C_, 4, 200).cpu().numpy(), want[1])
    assert np.array_equal(be.pattern(dev, A2, 4, 200).cpu().numpy(), want[0])
    assert np.array_equal(be.pattern(dev, B, 4, 200).cpu().numpy(), want[1])


def test_prepare_equals_the_lazy_path(gpu):
    import torch
    be, dl = gpu
    dev = torch.from_numpy(frames_of(256, 17, 33)).cuda()
    for gamma in (False, True):
        spec = dl.prepare_palette(palette_of(256), gamma)
        lazy, ahead = be.Palette(*spec), be.Palette(*spec)
        assert ahead.pattern_prepare() == (1 << 24) + 3 * 1024 == ahead.pattern_prepare()
        assert torch.equal(be.pattern(dev, ahead, 8, 128), be.pattern(dev, lazy, 8, 128)), gamma


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
        s = dl.PatternDitherStrategy("4x4", 0.5)
        d = dl.ImageDitherer(num_colors=16, dither_mode=s, palette=pal, use_gamma=gamma)
        pal_f32, outc, lut = dl.prepare_palette(pal, gamma)
        want = pr.pattern_u8(orc, arr, pal_f32, outc, lut, 4, 128)
        got = d.apply_dithering(img)
        assert got.mode == "RGB" and got.size == (33, 17) and np.array_equal(np.asarray(got), want), gamma
        p_img = d.apply_dithering_indexed(img)
        assert p_img.mode == "P" and np.array_equal(np.asarray(p_img.convert("RGB")), want), gamma
        png = d.apply_dithering_png(img)
        dec = Image.open(io.BytesIO(png))
        assert dec.mode == "P" and np.array_equal(np.asarray(dec.convert("RGB")), want), gamma
        # three frames through the video pipeline's batch functions
        frames = torch.from_numpy(np.stack([arr, arr[::-1].copy(), 255 - arr])).cuda()
        rgb = vp.process_frames(frames, d)
        assert np.array_equal(rgb[0].cpu().numpy(), want)
        planes, colours = vp.process_frames_indexed(frames, d)
        assert planes.shape == (3, 17, 33) and np.array_equal(colours[planes.cpu().numpy()], rgb.cpu().numpy()), gamma
    assert d.dither_mode is s                                           # the hook stores nothing and replaces nothing


def test_halftone_instance_through_the_hook(gpu):
    import torch
    be, dl = gpu
    frames = torch.from_numpy(frames_of(16, 67, 129)).cuda()
    pal = palette_of(16)
    h = dl.HalftoneDitherStrategy(cell_size=6, angle=30.0)
    d = dl.ImageDitherer(dither_mode=h, palette=pal)
    assert torch.equal(d.apply_dithering_frames(frames), h.dither_frames(frames, pal))
    with pytest.raises(ValueError, match="tiled"):
        d.apply_dithering_frames(frames, y0=4)
    with pytest.raises(NotImplementedError):
        dl.ImageDitherer(dither_mode=dl.DitherMode.HALFTONE, palette=pal).apply_dithering_frames(frames)
