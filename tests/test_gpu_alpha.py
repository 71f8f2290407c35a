"""GPU tier of transparency (include/ditherpie_hip_alpha.h): the split / key / join kernels and the two masked diffusions against
the numpy statements of tests/alpha_ref.py, bit for bit; the properties the masked kernels promise without a statement (an all-zero
mask is the unmasked call, masked output is `fill`, an opaque rectangle behind two masked pixels is the unmasked call on the crop,
hidden colours change nothing); the public layer (AlphaMode through ImageDitherer: RGBA, 'P' with transparency, PNG-8 with tRNS).
The diffusion references scan grey content on a black / white palette wherever the case is about the schedule and not about the
palette (the statement's memo then stays below 256 entries: tests/test_gpu_idiff.py), and colour content on small shapes where it is
about the palette.  A reference is computed once per case and shared (REF)."""
import ctypes as C
import io

import numpy as np
import pytest

import alpha_ref as ar
import dotdiff_ref as dr
import idiff_ref as ir

pytestmark = pytest.mark.gpu

REF = {}
BLACK_WHITE = [(0, 0, 0), (255, 255, 255)]
FILL = (7, 200, 33)


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


def palette_of(k):
    from test_gpu_pattern import palette_of as pattern_palette
    return pattern_palette(k)


def colour_frames(k, n, h, w):
    from test_gpu_pattern import frames_of as pattern_frames
    return np.ascontiguousarray(pattern_frames(k, h, w)[:n])


def grey_frames(n, h, w):
    rs = np.random.RandomState(7100 + 10 * h + w)
    v = rs.randint(0, 128, (n, h, w)) + (np.arange(w) * 127 // max(w - 1, 1))[None, None, :]
    return np.ascontiguousarray(np.repeat(v.astype(np.uint8)[..., None], 3, axis=-1))


def adapter(orc, metric):
    import metric_ref as mr
    return orc if metric == "rgb" else mr.NearestAdapter(metric)


def at_offset(t, off):
    """A copy of the CUDA tensor t whose first byte sits at an address = off (mod 16)."""
    import torch
    buf = torch.empty(t.numel() * t.element_size() + 32, dtype=torch.uint8, device=t.device)
    start = (off - buf.data_ptr()) % 16
    v = buf[start:start + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off
    return v


def to_cuda(a):
    """A (possibly read-only, shared) numpy array as a CUDA tensor of its own."""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def compare(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------------- split / key / join
def rgba_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    a = f[..., 3]
    a[rng.integers(0, 4, (n, h, w)) == 0] = 0                            # every alpha end value and the threshold's neighbours occur
    a[rng.integers(0, 4, (n, h, w)) == 0] = 255
    a[rng.integers(0, 8, (n, h, w)) == 0] = 127
    a[rng.integers(0, 8, (n, h, w)) == 0] = 128
    a[rng.integers(0, 16, (n, h, w)) == 0] = 1
    a[rng.integers(0, 16, (n, h, w)) == 0] = 254
    return f


SPLIT_SETTINGS = ([dict(mode="threshold", threshold=t) for t in (0, 1, 128, 255, 256)]
                  + [dict(mode="ordered", matrix=m, y0=y0, x0=x0) for m in (2, 4, 8) for y0, x0 in ((0, 0), (5, 3))])


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 19), (33, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n", [0, 3])
def test_split_matches_the_statement(gpu, shape, n):
    import torch
    be, _ = gpu
    h, w = shape
    src = rgba_frames(n, h, w, 10 * h + w)
    dev = torch.from_numpy(src).cuda()
    for i, kw in enumerate(SPLIT_SETTINGS):
        for matte in (None, (250, 10, 128)):
            ref_kw = {("m" if k == "matrix" else k): v for k, v in kw.items()}
            want = ar.split(src, matte=matte, **ref_kw)
            for off in (0, 1 + 2 * (i % 7)):                             # the dword instance (h * w % 4 == 0 only) and an odd address
                rgb, mask, masked = be.alpha_split(at_offset(dev, off) if n else dev, matte=matte, **kw)
                compare(rgb.cpu().numpy(), want[0], ("rgb", kw, matte, off))
                compare(mask.cpu().numpy(), want[1], ("mask", kw, matte, off))
                assert masked.dtype == torch.int64 and masked.cpu().tolist() == want[2].tolist(), (kw, matte, off)


def _raw_descriptors(be, _lib, rgba, rgb, mask, masked, planes, out, joined, kw):
    import torch
    L = _lib.load()
    n, h, w, _ = rgba.shape
    st = be._stream().value
    a = _lib.AlphaSplitArgs(C.sizeof(_lib.AlphaSplitArgs), rgba.data_ptr(), n, h, w, kw["mode"], kw["threshold"], kw["m"], kw["y0"], kw["x0"], 1,
                            _lib._rgb3(1, 2, 3), rgb.data_ptr(), mask.data_ptr(), masked.data_ptr(), st)
    assert L.dp_alpha_split_u8(C.byref(a)) == 0, L.dp_last_error()
    k = _lib.AlphaKeyArgs(C.sizeof(_lib.AlphaKeyArgs), planes.data_ptr(), mask.data_ptr(), n, h, w, 200, out.data_ptr(), st)
    assert L.dp_alpha_key_u8(C.byref(k)) == 0, L.dp_last_error()
    j = _lib.AlphaJoinArgs(C.sizeof(_lib.AlphaJoinArgs), rgb.data_ptr(), mask.data_ptr(), n, h, w, _lib._rgb3(*FILL), joined.data_ptr(), st)
    assert L.dp_alpha_join_u8(C.byref(j)) == 0, L.dp_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 19), (33, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("offs", [(0, 0, 0, 0, 0, 0), (1, 3, 5, 7, 9, 11), (4, 8, 12, 4, 8, 12), (4, 8, 13, 4, 8, 12)], ids=str)
def test_split_key_join_through_descriptors_at_every_alignment(gpu, shape, offs):
    """Every buffer at its own residue mod 16 (inputs AND outputs): all aligned, all odd, all dword-aligned, one odd among them."""
    import torch
    from dither_pie_amd import _lib
    be, _ = gpu
    h, w = shape
    n = 3
    src = rgba_frames(n, h, w, 77 + h)
    planes = np.random.default_rng(h).integers(0, 200, (n, h, w)).astype(np.uint8)
    rgba = at_offset(torch.from_numpy(src).cuda(), offs[0])
    rgb = at_offset(torch.full((n, h, w, 3), 0xAB, dtype=torch.uint8, device="cuda"), offs[1])
    mask = at_offset(torch.full((n, h, w), 0xCD, dtype=torch.uint8, device="cuda"), offs[2])
    masked = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    pl = at_offset(torch.from_numpy(planes).cuda(), offs[3])
    out = at_offset(torch.full((n, h, w), 0xEF, dtype=torch.uint8, device="cuda"), offs[4])
    joined = at_offset(torch.full((n, h, w, 4), 0x12, dtype=torch.uint8, device="cuda"), offs[5])
    kw = dict(mode=1, threshold=0, m=4, y0=9, x0=2)
    _raw_descriptors(be, _lib, rgba, rgb, mask, masked, pl, out, joined, kw)
    want = ar.split(src, "ordered", m=4, matte=(1, 2, 3), y0=9, x0=2)
    compare(rgb.cpu().numpy(), want[0], "rgb")
    compare(mask.cpu().numpy(), want[1], "mask")
    assert masked.cpu().tolist() == want[2].tolist()
    compare(out.cpu().numpy(), ar.key(planes, want[1], 200), "key")
    compare(joined.cpu().numpy(), ar.join(want[0], want[1], FILL), "join")


def test_key_in_place_and_join_and_any_nonzero_mask_byte(gpu):
    import torch
    be, _ = gpu
    rng = np.random.default_rng(3)
    for n, h, w in ((3, 17, 19), (2, 33, 128), (0, 4, 4)):
        planes = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
        rgb = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        mask = (rng.integers(0, 2, (n, h, w)) * rng.integers(1, 256, (n, h, w))).astype(np.uint8)
        p = torch.from_numpy(planes).cuda()
        k = to_cuda(mask)
        compare(be.alpha_key(p, k, 255).cpu().numpy(), ar.key(planes, mask, 255), "key")
        res = be.alpha_key(p, k, 0, out=p)                               # in place
        assert res.data_ptr() == p.data_ptr()
        compare(p.cpu().numpy(), ar.key(planes, mask, 0), "key in place")
        compare(be.alpha_join(torch.from_numpy(rgb).cuda(), k, FILL).cpu().numpy(), ar.join(rgb, mask, FILL), "join")
    with pytest.raises(ValueError):
        be.alpha_key(p.to(torch.int16), k, 3)


# ------------------------------------------------------------------------------------------------- masked integer error diffusion
SKEW1_TAPS = ([(-1, 2, 1)], 1)                                           # idiff_ref.tap_cases(): skew 1 with a left-pointing tap
IDIFF_TAPS = {"floyd_steinberg": ir.KERNELS["floyd_steinberg"], "atkinson": ir.KERNELS["atkinson"], "jjn": ir.KERNELS["jjn"], "skew1": SKEW1_TAPS}
IDIFF_SHAPES = [(1, 1), (3, 5), (64, 9), (65, 23), (130, 37), (1089, 5), (3, 7), (3, 8), (3, 16), (3, 17)]


def test_the_tap_sets_are_the_three_instances_and_a_skew_1_set():
    assert [len(IDIFF_TAPS[k][0]) for k in ("floyd_steinberg", "atkinson", "jjn")] == [4, 6, 12]
    assert (list(SKEW1_TAPS[0]), SKEW1_TAPS[1], 256) in [(list(t), d, s) for t, d, s in ir.tap_cases()] and ir.skew(SKEW1_TAPS[0]) == 1


def idiff_reference(orc, dl, tapname, shape, maskname):
    key = ("idiff", tapname, shape, maskname)
    if key not in REF:
        h, w = shape
        frame = grey_frames(1, h, w)[0]
        mask = ar.mask_family(maskname, h, w, seed=h + w)
        spec = dl.prepare_palette(BLACK_WHITE, False)
        REF[key] = (frame, mask, ar.idiff_masked_u8(orc, frame, mask, *spec, *IDIFF_TAPS[tapname], 256, FILL))
        for a in REF[key]:
            a.setflags(write=False)
    return REF[key]


@pytest.mark.parametrize("tapname", sorted(IDIFF_TAPS))
@pytest.mark.parametrize("shape", IDIFF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_idiff_matches_the_statement_at_every_shape(gpu, orc, shape, tapname):
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(BLACK_WHITE, False))
    for maskname in ("half", "sixteenth"):
        frame, mask, want = idiff_reference(orc, dl, tapname, shape, maskname)
        got = be.idiff_masked(to_cuda(frame), to_cuda(mask), P, *IDIFF_TAPS[tapname], 256, fill=FILL)
        compare(got.cpu().numpy(), want, (tapname, shape, maskname))


@pytest.mark.parametrize("maskname", ar.MASKS)
def test_masked_idiff_matches_the_statement_for_every_mask(gpu, orc, maskname):
    """Three bands and the hand-off rows (130 x 37), Floyd-Steinberg and JJN (two rows of reach across the band edge)."""
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(BLACK_WHITE, False))
    for tapname in ("floyd_steinberg", "jjn"):
        frame, mask, want = idiff_reference(orc, dl, tapname, (130, 37), maskname)
        got = be.idiff_masked(to_cuda(frame), to_cuda(mask), P, *IDIFF_TAPS[tapname], 256, fill=FILL)
        compare(got.cpu().numpy(), want, (tapname, maskname))
        if maskname == "transparent":
            assert (got.cpu().numpy() == np.array(FILL, np.uint8)).all()


@pytest.mark.parametrize("what", ["gamma16", "oklab16", "rgb256"])
def test_masked_idiff_palettes_and_a_batch_with_different_masks(gpu, orc, what):
    import torch
    be, dl = gpu
    k, gamma, metric = {"gamma16": (16, True, "rgb"), "oklab16": (16, False, "oklab"), "rgb256": (256, False, "rgb")}[what]
    spec = dl.prepare_palette(palette_of(k), gamma)
    assert (spec[2] is not None) == gamma
    P = be.Palette(*spec, metric=metric) if metric != "rgb" else be.Palette(*spec)
    n, h, w = 3, 20, 23
    frames = colour_frames(k, n, h, w)
    masks = np.stack([ar.mask_family(m, h, w, seed=5) for m in ("half", "sixteenth", "checker")])
    taps, div = ir.KERNELS["floyd_steinberg"]
    want = np.stack([ar.idiff_masked_u8(adapter(orc, metric), f, m, *spec, taps, div, 256, FILL) for f, m in zip(frames, masks)])
    got = be.idiff_masked(torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda(), P, taps, div, 256, fill=FILL)
    compare(got.cpu().numpy(), want, what)


# ------------------------------------------------------------------------------------------------- masked dot diffusion
def matrix16():
    """A 16 x 16 class matrix of reach <= 16: the Bayer rank recursion taken one step further (its reach is 3, as Bayer 8's)."""
    b = ar.bayer_rank(8)
    return np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])


def reach16(m):
    """A seeded random m x m class matrix whose reach is exactly 16, the largest the kernel takes: dependency chains as long as the
    halo, which is what the mask bytes read beyond a tile's region are for."""
    return np.random.RandomState({8: 26, 16: 2}[m]).permutation(m * m).reshape(m, m).astype(np.int64)


def dot_matrices():
    return {"knuth": dr.KNUTH, "bayer2": ar.bayer_rank(2), "bayer4": ar.bayer_rank(4), "m16": matrix16(), "reach16_8": reach16(8),
            "reach16_16": reach16(16)}


def test_the_16_wide_matrix_is_within_reach_and_two_matrices_reach_the_limit():
    assert sorted(matrix16().reshape(-1).tolist()) == list(range(256)) and dr.reach(matrix16()) <= dr.MAX_REACH
    assert dr.reach(reach16(8)) == dr.reach(reach16(16)) == dr.MAX_REACH == 16


def dotdiff_reference(orc, dl, mname, shape, maskname):
    key = ("dot", mname, shape, maskname)
    if key not in REF:
        h, w = shape
        frame = grey_frames(1, h, w)[0]
        mask = ar.mask_family(maskname, h, w, seed=2 * h + w)
        spec = dl.prepare_palette(BLACK_WHITE, False)
        REF[key] = (frame, mask, ar.dotdiff_masked_u8(orc, frame, mask, *spec, dot_matrices()[mname], 256, FILL))
        for a in REF[key]:
            a.setflags(write=False)
    return REF[key]


@pytest.mark.parametrize("mname", ["knuth", "bayer2", "bayer4", "m16"])
@pytest.mark.parametrize("shape", [(1, 1), (15, 17), (64, 64), (65, 81), (130, 97)], ids=lambda s: "x".join(map(str, s)))
def test_masked_dotdiff_matches_the_statement_at_every_shape(gpu, orc, shape, mname):
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(BLACK_WHITE, False))
    for maskname in ("half", "sixteenth"):
        frame, mask, want = dotdiff_reference(orc, dl, mname, shape, maskname)
        got = be.dotdiff_masked(to_cuda(frame), to_cuda(mask), P, dot_matrices()[mname], 256, fill=FILL)
        compare(got.cpu().numpy(), want, (mname, shape, maskname))


@pytest.mark.parametrize("maskname", ar.MASKS)
def test_masked_dotdiff_matches_the_statement_for_every_mask(gpu, orc, maskname):
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(BLACK_WHITE, False))
    frame, mask, want = dotdiff_reference(orc, dl, "knuth", (65, 81), maskname)
    got = be.dotdiff_masked(to_cuda(frame), to_cuda(mask), P, dr.KNUTH, 256, fill=FILL)
    compare(got.cpu().numpy(), want, maskname)


@pytest.mark.parametrize("mname", ["reach16_8", "reach16_16"])
def test_masked_dotdiff_at_the_largest_reach(gpu, orc, mname):
    """Matrices of reach 16 on three tiles by two: a pixel of the tile's first row or column may hang on a chain that starts on the
    region's edge, whose W depends on mask bytes beyond the region.  Every mask of the family, and the unmasked kernel beside it."""
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(BLACK_WHITE, False))
    M = dot_matrices()[mname]
    assert be.dotdiff_reach(M) == 16
    for maskname in ("half", "sixteenth", "checker", "opaque"):
        frame, mask, want = dotdiff_reference(orc, dl, mname, (130, 97), maskname)
        got = be.dotdiff_masked(to_cuda(frame), to_cuda(mask), P, M, 256, fill=FILL)
        compare(got.cpu().numpy(), want, (mname, maskname))
        if maskname == "opaque":
            assert torch.equal(got, be.dotdiff(to_cuda(frame), P, M, 256))


def test_masked_dotdiff_colour_palettes_and_a_batch(gpu, orc):
    import torch
    be, dl = gpu
    for k, gamma in ((16, True), (256, False)):
        spec = dl.prepare_palette(palette_of(k), gamma)
        P = be.Palette(*spec)
        n, h, w = 3, 18, 21
        frames = colour_frames(k, n, h, w)
        masks = np.stack([ar.mask_family(m, h, w, seed=9) for m in ("half", "sixteenth", "checker")])
        want = np.stack([ar.dotdiff_masked_u8(orc, f, m, *spec, dr.KNUTH, 200, FILL) for f, m in zip(frames, masks)])
        got = be.dotdiff_masked(torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda(), P, dr.KNUTH, 200, fill=FILL)
        compare(got.cpu().numpy(), want, (k, gamma))


# ------------------------------------------------------------------------------------------------- properties of the kernels
def _runners(be, P):
    taps, div = ir.KERNELS["jjn"]
    return {
        "idiff": (lambda f, k: be.idiff_masked(f, k, P, taps, div, 256, fill=FILL), lambda f: be.idiff(f, P, taps, div, 256), 1),
        "dotdiff": (lambda f, k: be.dotdiff_masked(f, k, P, dr.KNUTH, 256, fill=FILL), lambda f: be.dotdiff(f, P, dr.KNUTH, 256), 8),
    }


@pytest.mark.parametrize("which", ["idiff", "dotdiff"])
def test_properties_of_the_masked_kernels(gpu, which):
    import torch
    be, dl = gpu
    P = be.Palette(*dl.prepare_palette(palette_of(16), False))
    masked, plain, grid = _runners(be, P)[which]
    n, h, w = 2, 150, 170
    frames = colour_frames(16, n, h, w)
    dev = torch.from_numpy(frames).cuda()
    # an all-zero mask is the unmasked call
    zero = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    assert torch.equal(masked(dev, zero), plain(dev))
    # fill exactly where the mask is set; hidden colours change nothing
    mask = np.stack([ar.mask_family("half", h, w, seed=1), ar.mask_family("sixteenth", h, w, seed=2)])
    k = to_cuda(mask)
    a = masked(dev, k).cpu().numpy()
    assert (a[mask != 0] == np.array(FILL, np.uint8)).all()
    other = frames.copy()
    other[mask != 0] = np.random.default_rng(4).integers(0, 256, (int((mask != 0).sum()), 3)).astype(np.uint8)
    assert not np.array_equal(other, frames)
    b = masked(torch.from_numpy(other).cuda(), k).cpu().numpy()
    assert np.array_equal(a, b)
    # isolation: opaque rectangles behind two masked pixels on every side that is not a frame edge come out as the unmasked call on
    # the crop; one straddles row 64 (the band hand-off), one the tile edge at column 64, one touches the frame's corner
    rects = [(56, 16, 80, 40), (16, 56, 40, 88), (0, 0, 8, 8), (128, 96, 150, 170)]     # y0, x0, y1, x1: origins multiples of 8
    iso = np.ones((1, h, w), np.uint8)
    for y0, x0, y1, x1 in rects:
        assert y0 % grid == 0 and x0 % grid == 0
        iso[0, y0:y1, x0:x1] = 0
    got = masked(dev[:1], torch.from_numpy(iso).cuda()).cpu().numpy()[0]
    for y0, x0, y1, x1 in rects:
        alone = plain(torch.from_numpy(np.ascontiguousarray(frames[0, y0:y1, x0:x1])).cuda()).cpu().numpy()
        compare(got[y0:y1, x0:x1], alone, (which, y0, x0))


# ------------------------------------------------------------------------------------------------- the public layer
def sprite():
    """A 40 x 56 RGBA sprite: a disc with a soft edge on a transparent ground whose hidden colours are loud and many."""
    h, w = 40, 56
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.hypot(yy - 19.5, (xx - 27.5) * 0.75)
    alpha = np.clip((17.0 - d) * 64.0, 0, 255).astype(np.uint8)           # four pixels of ramp
    rng = np.random.default_rng(11)
    rgb = np.empty((h, w, 3), np.uint8)
    rgb[...] = (200, 60, 40)
    rgb[yy > 20] = (230, 200, 60)
    rgb[(xx // 4 + yy // 4) % 3 == 0] = (120, 30, 30)
    hidden = alpha == 0
    rgb[hidden] = rng.integers(0, 256, (int(hidden.sum()), 3)).astype(np.uint8) & 0xF0 | 0x0F    # blues and greens nobody sees
    return np.dstack([rgb, alpha])


def alpha_modes(dl):
    return [dl.AlphaMode(), dl.AlphaMode(mode="ordered", matrix="4x4", matte=(255, 255, 255), fill=(1, 2, 3)),
            dl.AlphaMode(mode="threshold", threshold=1, matte=(0, 0, 0), fill=(255, 0, 255))]


@pytest.mark.parametrize("strategy", ["bayer", "idiff", "dotdiff"])
def test_rgba_p_and_png_are_one_image(gpu, strategy):
    from PIL import Image
    be, dl = gpu
    src = sprite()
    image = Image.fromarray(src, "RGBA")
    mode = {"bayer": dl.DitherMode.BAYER, "idiff": dl.IntegerErrorDiffusionDitherStrategy(), "dotdiff": dl.DotDiffusionDitherStrategy()}[strategy]
    for am in alpha_modes(dl):
        d = dl.ImageDitherer(num_colors=8, dither_mode=mode, palette=None)
        rgba = d.apply_dithering_rgba(image, alpha=am)
        assert rgba.mode == "RGBA" and rgba.size == image.size
        p = d.apply_dithering_indexed_alpha(image, alpha=am)
        K = len(d.palette)
        assert p.mode == "P" and p.info["transparency"] == K
        png = Image.open(io.BytesIO(d.apply_dithering_png(image, alpha=am)))
        assert png.mode == "P" and png.info["transparency"] == K
        a = np.asarray(rgba)
        compare(np.asarray(p.convert("RGBA")), a, (strategy, am, "P"))
        compare(np.asarray(png.convert("RGBA")), a, (strategy, am, "png"))
        if am.mode == "ordered":                                         # the chunk is part of the device-assembled prefix too
            dev = Image.open(io.BytesIO(d.apply_dithering_png(image, blocks="dynamic", assemble="device", alpha=am)))
            assert dev.info["transparency"] == K
            compare(np.asarray(dev.convert("RGBA")), a, (strategy, am, "png, assembled on the device"))
        m = ar.mask_of(src[..., 3], am.mode, am.threshold, int(str(am.matrix).split("x")[0]))
        assert np.array_equal(a[..., 3] == 0, m != 0) and set(np.unique(a[..., 3]).tolist()) <= {0, 255}
        assert (a[m != 0, :3] == np.array(am.fill, np.uint8)).all()
        assert 0 < (m != 0).sum() < m.size


def test_the_palette_is_fitted_to_what_can_be_seen(gpu):
    from PIL import Image
    be, dl = gpu
    src = sprite()
    image = Image.fromarray(src, "RGBA")
    am = dl.AlphaMode(matte=(255, 255, 255))
    d = dl.ImageDitherer(num_colors=8, dither_mode=dl.DitherMode.BAYER, palette=None)
    d.apply_dithering_rgba(image, alpha=am)
    rgb, mask, _ = ar.split(src[None], "threshold", 128, matte=am.matte)
    seen = np.ascontiguousarray(rgb[0][mask[0] == 0].reshape(1, -1, 3))
    e = dl.ImageDitherer(num_colors=8, dither_mode=dl.DitherMode.BAYER, palette=None)
    e._ensure_palette(seen)
    assert d.palette == e.palette
    f = dl.ImageDitherer(num_colors=8, dither_mode=dl.DitherMode.BAYER, palette=None)
    f._ensure_palette(np.ascontiguousarray(src[..., :3]))
    assert f.palette != d.palette                                        # alpha ignored: entries spent on the hidden colours
    # the existing call is what it was: alpha dropped by convert("RGB"), no tRNS
    g = dl.ImageDitherer(num_colors=8, dither_mode=dl.DitherMode.BAYER, palette=f.palette)
    data = g.apply_dithering_png(image)
    assert b"tRNS" not in data and data == g.apply_dithering_png(image.convert("RGB"))
    # ... pinned independently of apply_dithering_png: the 'P' image of the existing path, encoded by png.encode_png without the keyword
    import torch
    from dither_pie_amd import png
    p = g.apply_dithering_indexed(image)
    colours = dl.prepare_palette(g.palette, False)[1]
    assert "transparency" not in p.info and np.array_equal(np.asarray(p.getpalette()[:3 * len(colours)], np.uint8).reshape(-1, 3), colours)
    planes = torch.from_numpy(np.array(p)).cuda()
    depth = be.png_depth(len(colours))
    assert data == png.encode_png(planes, colours)[0] == png.container(56, 40, depth, colours, be.png_deflate_host(np.array(p)[None], depth)[0])


@pytest.mark.parametrize("strategy", ["bayer", "idiff"])
def test_an_image_without_an_opaque_pixel_has_nothing_to_fit(gpu, strategy):
    """palette=None and alpha 0 everywhere: ValueError from every public call, and the ditherer is left without a palette."""
    from PIL import Image
    be, dl = gpu
    src = sprite()
    src[..., 3] = 0
    image = Image.fromarray(src, "RGBA")
    mode = {"bayer": dl.DitherMode.BAYER, "idiff": dl.IntegerErrorDiffusionDitherStrategy()}[strategy]
    d = dl.ImageDitherer(num_colors=8, dither_mode=mode, palette=None)
    for am in (dl.AlphaMode(), dl.AlphaMode(mode="ordered", matte=(255, 255, 255))):
        for call in (lambda: d.apply_dithering_rgba(image, alpha=am), lambda: d.apply_dithering_indexed_alpha(image, alpha=am),
                     lambda: d.apply_dithering_png(image, alpha=am), lambda: d.apply_dithering_frames_alpha(torch_rgba(src), am),
                     lambda: d.apply_dithering_frames_indexed_alpha(torch_rgba(src), am)):
            with pytest.raises(ValueError, match="opaque pixel"):
                call()
            assert d.palette is None
    # one opaque pixel is enough; and with a palette given there is nothing to fit, so an all-transparent image is fine
    src[3, 4, 3] = 255
    one = d.apply_dithering_rgba(Image.fromarray(src, "RGBA"))
    assert d.palette is not None and (np.asarray(one)[..., 3] == 255).sum() == 1
    src[..., 3] = 0
    out = np.asarray(d.apply_dithering_rgba(Image.fromarray(src, "RGBA")))
    assert (out == 0).all()


def torch_rgba(src):
    import torch
    return torch.from_numpy(np.array(src)).cuda()
