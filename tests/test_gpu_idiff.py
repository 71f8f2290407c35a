"""GPU tier of integer error diffusion: byte equality of dp_idiff_u8 (through backend.idiff, IntegerErrorDiffusionDitherStrategy
and the instance hook of ImageDitherer) with the push-form statement tests/idiff_ref.py, which scans pixel by pixel and knows
nothing of bands, skews, rings or periods -- under the RGB metric (the CPU oracle's nearest) and under Oklab
(metric_ref.NearestAdapter).  The shapes are the smallest at which the schedule can go wrong (SHAPES below says what each is
for).  A reference is computed once per case and shared (REF).  The references of this file scan about 480 000 pixels in all
(the file takes about 12 s on an MI355X machine, 8 s before the last three groups below were added): the shapes, the eight
variants on (2, 70, 37), the palette sizes and the strengths, each under both metrics, 0.1 to 0.5 s per 5 000 pixels of 16-colour
content, 165 000 pixels; the tap sets of idiff_ref.tap_cases() on (1, 66, 21), 58 000 pixels, 1.6 s; and grey content on a
black / white palette, where every query of the statement is a grey and its memo stays small: three frames of 192 rows that put
two bands on the workspace at once and one of 1030 rows, 256 000 pixels, 1.5 s.  No case takes more than a second."""
import io

import numpy as np
import pytest

import idiff_ref as ir

pytestmark = pytest.mark.gpu

PERIOD, OTHER_PERIOD = 8, 16                                            # idiff.hip: kIdPeriod (checked below), and what DP_IDIFF_PERIOD selects
SHAPES = [
    (1, 1, 1), (1, 1, 7), (2, 3, 2),                                    # no row above; narrower than the taps reach
    (3, 17, 33),                                                        # the plain case, several frames
    (1, 64, 9), (1, 65, 9),                                             # the band edge
    (2, 130, 70),                                                       # three bands, wider than the 64-column ring, two frames
    (1, 5, 200),                                                        # many periods, few rows
    (1, 1030, 3),                                                       # 17 bands: more than a workgroup has waves, a wave takes a second band
    (1, 3, PERIOD - 1), (1, 3, PERIOD), (1, 3, PERIOD + 1),             # widths around the I/O period
    (1, 3, OTHER_PERIOD - 1), (1, 3, OTHER_PERIOD), (1, 3, OTHER_PERIOD + 1),   # ... and around the other period length
]
METRICS = ("rgb", "oklab")
REF = {}


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
    """The palette list (RGB triples) of the K cases (those of tests/test_gpu_pattern.py; 5: duplicate entries, 2: a real tie)."""
    from test_gpu_pattern import palette_of as pattern_palette
    return pattern_palette(k)


def frames_of(k, n, h, w):
    """n <= 3 distinct frames: noise, a gradient with noise, dark noise (tests/test_gpu_pattern.py)."""
    from test_gpu_pattern import frames_of as pattern_frames
    return np.ascontiguousarray(pattern_frames(k, h, w)[:n])


def adapter(orc, metric):
    import metric_ref as mr
    return orc if metric == "rgb" else mr.NearestAdapter(metric)


def reference(orc, metric, frames, spec, name, s, key):
    full = (metric, name, s) + key
    if full not in REF:
        REF[full] = ir.idiff_frames(adapter(orc, metric), frames, *spec, *ir.KERNELS[name], s)
        REF[full].setflags(write=False)
    return REF[full]


def device_palette(be, spec, metric):
    pal_f32, outc, lut = spec
    return be.Palette(pal_f32, outc, lut, metric=metric) if metric != "rgb" else be.Palette(pal_f32, outc, lut)


def compare(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert not len(bad), (what, len(bad), bad[:4].tolist())


BLACK_WHITE = [(0, 0, 0), (255, 255, 255)]


def grey_frames(n, h, w):
    """Grey frames (r = g = b): seeded noise plus a horizontal ramp.  With BLACK_WHITE every query of the statement is (v, v, v),
    so its memo holds at most 256 entries and the serial scan stays cheap at sizes the colour cases cannot afford."""
    rs = np.random.RandomState(7000 + 10 * h + w)
    v = rs.randint(0, 128, (n, h, w)) + (np.arange(w) * 127 // max(w - 1, 1))[None, None, :]
    return np.ascontiguousarray(np.repeat(v.astype(np.uint8)[..., None], 3, axis=-1))


def grey_case(orc, dl, taps, divisor, shape):
    """-> (palette spec, frames, the statement's output) of a grey case at strength 256, computed once."""
    spec = dl.prepare_palette(BLACK_WHITE, False)
    key = ("grey", tuple(taps), divisor, shape)
    if key not in REF:
        frames = grey_frames(*shape)
        REF[key] = (frames, ir.idiff_frames(orc, frames, *spec, taps, divisor, 256))
        REF[key][1].setflags(write=False)
        assert 0.2 < (REF[key][1] == 255).mean() < 0.8                  # both colours, neither rare
    return (spec,) + REF[key]


def test_the_period_is_the_kernels():
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "dither_pie_amd", "csrc", "idiff.hip")) as f:
        assert int(re.search(r"constexpr int kIdPeriod = (\d+);", f.read()).group(1)) == PERIOD


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_statement_at_every_shape(gpu, orc, shape, metric):
    import torch
    be, dl = gpu
    n, h, w = shape
    spec = dl.prepare_palette(palette_of(16), False)
    P = device_palette(be, spec, metric)
    frames = frames_of(16, n, h, w)
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    want = reference(orc, metric, frames, spec, "floyd_steinberg", 256, ("shape", shape))
    dev = torch.from_numpy(frames).cuda()
    compare(be.idiff(dev, P, taps, divisor, 256).cpu().numpy(), want, (shape, metric))
    if n > 1:                                                           # a batch equals its frames one by one
        compare(be.idiff(dev[1:2].clone(), P, taps, divisor, 256).cpu().numpy(), want[1:2], (shape, metric, "N = 1"))
    del P


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", sorted(ir.KERNELS))
def test_all_eight_variants(gpu, orc, name, metric):
    """(2, 70, 37): two bands, a width that is no multiple of anything, two frames; skew 2 and skew 3; 3 to 12 taps."""
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(palette_of(16), False)
    P = device_palette(be, spec, metric)
    frames = frames_of(16, 2, 70, 37)
    want = reference(orc, metric, frames, spec, name, 256, ("variants",))
    got = dl.IntegerErrorDiffusionDitherStrategy(name)._run(torch.from_numpy(frames).cuda(), P).cpu().numpy()
    compare(got, want, (name, metric))
    del P


TAP_CASES = ir.tap_cases()
TAP_RUNS = [(i, "rgb") for i in range(len(TAP_CASES))] + [(i, "oklab") for i in range(0, len(TAP_CASES), 4)]


@pytest.mark.parametrize("i,metric", TAP_RUNS, ids=lambda v: str(v))
def test_tap_sets_beyond_the_variants(gpu, orc, i, metric):
    """idiff_ref.tap_cases() (tests/test_idiff_cpu.py says what the list covers: skew 1, every tap count 1 .. 12, spare slots in
    each instance, a two-tap set at the ring depth) at (1, 66, 21): rows 62 .. 65 cross the band edge, and 21 columns are more
    than the 8-column ring and the 8-step period hold.  Every case under RGB, every fourth under Oklab."""
    import torch
    be, dl = gpu
    taps, divisor, s = TAP_CASES[i]
    spec = dl.prepare_palette(palette_of(16), False)
    P = device_palette(be, spec, metric)
    frames = frames_of(16, 1, 66, 21)
    want = ir.idiff_frames(adapter(orc, metric), frames, *spec, taps, divisor, s)
    got = be.idiff(torch.from_numpy(frames).cuda(), P, taps, divisor, s).cpu().numpy()
    compare(got, want, (i, taps, divisor, s, ir.skew(taps), metric))
    del P


FS4_SKEW_1 = ([(1, 0, 7), (0, 1, 5), (1, 1, 3), (0, 2, 1)], 16)
TWO_BANDS_ON_THE_WORKSPACE = [(FS4_SKEW_1, 1, (1, 192, 192)), (ir.KERNELS["floyd_steinberg"], 2, (1, 192, 320)), (ir.KERNELS["jjn"], 3, (1, 192, 448))]


@pytest.mark.parametrize("kernel,skew,shape", TWO_BANDS_ON_THE_WORKSPACE, ids=["skew1-192x192", "skew2-192x320", "skew3-192x448"])
def test_two_bands_on_the_workspace_at_once(gpu, orc, kernel, skew, shape):
    """Band b + 2 stores its boundary rows into the buffer band b wrote while band b + 1 still prefetches from that buffer.

    From idiff.hip as it stands (P = kIdPeriod = 8, s = the skew, steps counted on each wave's own clock t0):
      * lane 62 of band b + 2 works on column 0 at step 62 s; the errors of that period go to the workspace at the boundary
        T = P * floor(62 s / P) + P <= 62 s + P.  The store comes before that boundary's own wait, so the wave only had to pass
        the wait of boundary T - P, which asks band b + 1 for need = T + P + 2 columns of its rows 62 / 63;
      * band b + 1 publishes t0 - P - 63 s columns at its boundary t0: at the first store of band b + 2 it is at
        t0 >= T + 2 P + 2 + 63 s, the next boundary being at most 125 s + 4 P + 1 = 125 s + 33 (152, 272 and 400 for s = 1, 2, 3);
      * band b + 1 issues a prefetch at every boundary with t0 + 2 P + 2 - 32 < w, that is t0 < w + 14;
      * so both happen in the same stretch of time only for w > 125 s + 20, and only where band b + 2 has rows 62 and 63:
        h >= 192.  The widths here leave 47, 50 and 53 columns beyond that, five I/O periods and more: the step counts are
        read from the code, nobody has measured them.
    The widest multi-band shape of SHAPES, (130, 70), has a two-row third band that stores nothing.

    Grey content and a black / white palette keep the serial statement cheap (grey_frames) -- and are blind to a swapped
    channel: channel handling at band edges stays with the colour cases (2, 130, 70) and (2, 70, 37).  The overlap depends on
    the waves running close to their minimum distance, which nothing forces: the test can catch a store of band b + 2 that
    lands where band b + 1 has yet to read, it cannot prove there is none.

    What it cannot catch, by the same arithmetic: a kernel whose bands all use ONE buffer.  A band fetches column c for the last
    time at its boundary t0 <= c + 30 - 2 P = c + 14 and stores its own column c after step c + 62 s, and the band below reads
    that column only once it is published: per column the order is write, read, overwrite, read, whichever bands run together.
    A library built with bprev and bnext on the same buffer passed this test, every other test of this file and frames up to
    1024 columns wide on an MI355X: in pixels the second buffer is spare."""
    import torch
    be, dl = gpu
    taps, divisor = kernel
    n, h, w = shape
    assert ir.skew(taps) == skew and sum(wt for _, _, wt in taps) == divisor
    assert w > 125 * ir.skew(taps) + 20 and h >= 192
    assert w - (125 * ir.skew(taps) + 20) >= 5 * PERIOD
    spec, frames, want = grey_case(orc, dl, taps, divisor, shape)
    P = be.Palette(*spec)
    compare(be.idiff(torch.from_numpy(frames).cuda(), P, taps, divisor, 256).cpu().numpy(), want, (shape, skew))
    del P


SECOND_BAND_WIDE = (1, 1030, 70)


def test_a_waves_second_band_with_real_width(gpu, orc):
    """(1, 1030, 70): 17 bands for 16 waves as in (1, 1030, 3), but wave 0's second band wraps the 64-column ring of the rows
    above it and runs full I/O periods.  Grey content, black / white palette (grey_frames)."""
    import torch
    be, dl = gpu
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    spec, frames, want = grey_case(orc, dl, taps, divisor, SECOND_BAND_WIDE)
    P = be.Palette(*spec)
    compare(be.idiff(torch.from_numpy(frames).cuda(), P, taps, divisor, 256).cpu().numpy(), want, SECOND_BAND_WIDE)
    del P


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 2, 5, 256])
def test_palette_sizes_and_a_duplicate_entry(gpu, orc, k, metric):
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(palette_of(k), False)
    assert spec[0].shape == (k, 3)
    P = device_palette(be, spec, metric)
    frames = frames_of(k, 3, 17, 33)
    want = reference(orc, metric, frames, spec, "sierra", 256, ("k", k))
    compare(be.idiff(torch.from_numpy(frames).cuda(), P, *ir.KERNELS["sierra"], 256).cpu().numpy(), want, (k, metric))
    del P


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("s", [0, 77, 256])
def test_strengths(gpu, orc, s, metric):
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(palette_of(16), False)
    P = device_palette(be, spec, metric)
    frames = frames_of(16, 3, 17, 33)
    dev = torch.from_numpy(frames).cuda()
    want = reference(orc, metric, frames, spec, "jjn", s, ("strength",))
    got = be.idiff(dev, P, *ir.KERNELS["jjn"], s)
    compare(got.cpu().numpy(), want, (s, metric))
    if s == 0:                                                          # strength 0 is the nearest-only mode of the device, too
        none = dl.ImageDitherer(dither_mode=dl.DitherMode.NONE, palette=palette_of(16), metric=metric).apply_dithering_frames(dev)
        assert torch.equal(got, none)
    del P


@pytest.mark.parametrize("name", ["floyd_steinberg", "stucki"])
def test_gamma_goes_through_lut_in(gpu, orc, name):
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(palette_of(16), True)
    assert spec[2] is not None
    frames = frames_of(16, 3, 17, 33)
    want = reference(orc, "rgb", frames, spec, name, 256, ("gamma",))
    got = dl.IntegerErrorDiffusionDitherStrategy(name).dither_frames(torch.from_numpy(frames).cuda(), palette_of(16), use_gamma=True)
    compare(got.cpu().numpy(), want, name)
    assert not np.array_equal(want, reference(orc, "rgb", frames, dl.prepare_palette(palette_of(16), False), name, 256, ("no gamma",)))


def test_stale_scratch_two_shapes_back_to_back(gpu, orc):
    """Two calls of different shape on one stream with one workspace that held 0xFF: the second equals a fresh run."""
    import torch
    be, dl = gpu
    from dither_pie_amd import _lib
    L = _lib.load()
    spec = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(*spec)
    P.pattern_prepare()
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))
    calls = []
    for n, h, w in ((2, 130, 70), (3, 17, 33)):
        frames = frames_of(16, n, h, w)
        calls.append((frames, torch.from_numpy(frames).cuda(), torch.full(frames.shape, 0xA5, dtype=torch.uint8, device="cuda"),
                      reference(orc, "rgb", frames, spec, "floyd_steinberg", 256, ("shape", (n, h, w)))))
    need = max(L.dp_idiff_workspace_bytes(*f.shape[:3]) for f, _, _, _ in calls)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for frames, dev, out, _ in calls:                                   # no synchronisation in between
        n, h, w, _c = frames.shape
        rc = L.dp_idiff_u8(dev.data_ptr(), out.data_ptr(), n, h, w, P._h, dx.ctypes.data, dy.ctypes.data, wt.ctypes.data, len(taps), divisor, 256,
                           ws.data_ptr(), ws.numel(), be._stream())
        assert rc == 0, L.dp_last_error()
    torch.cuda.synchronize()
    for frames, _, out, want in calls:
        compare(out.cpu().numpy(), want, frames.shape)
    del P


def test_repeatable_out_buffers_and_refusals(gpu):
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(*spec)
    frames = torch.from_numpy(frames_of(16, 3, 17, 33)).cuda()
    fs = ir.KERNELS["floyd_steinberg"]
    want = be.idiff(frames, P, *fs, 256)
    assert torch.equal(be.idiff(frames, P, *fs, 256), want) and not torch.equal(want[0], want[1])
    one = be.idiff(frames[2], P, *fs, 256)                              # [H,W,3]
    assert one.shape == frames[2].shape and torch.equal(one, want[2])
    buf = torch.full_like(frames, 0xAB)
    got = be.idiff(frames, P, *fs, 256, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    keep = frames.clone()
    with pytest.raises(ValueError, match="in place"):
        be.idiff(frames, P, *fs, 256, out=frames)
    assert torch.equal(frames, keep)
    s = dl.IntegerErrorDiffusionDitherStrategy()
    assert torch.equal(s.dither_frames(frames, palette_of(16)), want)
    planes, colours = s.dither_frames_indexed(frames, palette_of(16))
    assert planes.dtype == torch.uint8 and planes.shape == frames.shape[:3]
    assert np.array_equal(colours[planes.cpu().numpy()], want.cpu().numpy())
    with pytest.raises(ValueError, match="tiled"):
        s._run(frames, P, y0=8)
    px = frames[0].cpu().numpy().reshape(-1, 3).astype(np.float32)      # the strategy contract of the reference
    back = s.dither(px, np.array(palette_of(16), np.float32), (17, 33))
    assert back.shape == px.shape and np.array_equal(back.astype(np.uint8).reshape(17, 33, 3), want[0].cpu().numpy())
    # the float scan still refuses a metric palette; this scan takes it
    M = be.Palette(spec[0], spec[1], metric="oklab")
    with pytest.raises((ValueError, be.DitherPieError)):
        be.error_diffusion(frames, M, fs[0], fs[1])
    assert not torch.equal(be.idiff(frames, M, *fs, 256), want)
    del P, M


@pytest.mark.parametrize("shape", [(2, 130, 70), (1, 3, OTHER_PERIOD - 1), (1, 3, OTHER_PERIOD), (1, 3, OTHER_PERIOD + 1), (1, 1030, 3)], ids=lambda s: "x".join(map(str, s)))
def test_the_other_period_length(gpu, orc, switches, shape):
    """The experiments library with 16-step I/O periods (the A/B of DESIGN.md 4.3i): the same bytes."""
    import torch
    be, dl = gpu
    switches.setenv("DP_IDIFF_PERIOD", str(OTHER_PERIOD))
    n, h, w = shape
    spec = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(*spec)
    frames = frames_of(16, n, h, w)
    want = reference(orc, "rgb", frames, spec, "floyd_steinberg", 256, ("shape", shape))
    compare(be.idiff(torch.from_numpy(frames).cuda(), P, *ir.KERNELS["floyd_steinberg"], 256).cpu().numpy(), want, shape)
    del P


def test_the_other_period_length_on_a_waves_second_band_with_real_width(gpu, orc, switches):
    """(1, 1030, 70) of test_a_waves_second_band_with_real_width with 16-step periods: the same bytes."""
    import torch
    be, dl = gpu
    switches.setenv("DP_IDIFF_PERIOD", str(OTHER_PERIOD))
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    spec, frames, want = grey_case(orc, dl, taps, divisor, SECOND_BAND_WIDE)
    P = be.Palette(*spec)
    compare(be.idiff(torch.from_numpy(frames).cuda(), P, taps, divisor, 256).cpu().numpy(), want, SECOND_BAND_WIDE)
    del P


def test_the_other_period_length_with_every_variant(gpu, orc, switches):
    """... and the three tap-slot instances of that period, on the shape and the references of test_all_eight_variants."""
    import torch
    be, dl = gpu
    switches.setenv("DP_IDIFF_PERIOD", str(OTHER_PERIOD))
    spec = dl.prepare_palette(palette_of(16), False)
    P = be.Palette(*spec)
    frames = frames_of(16, 2, 70, 37)
    dev = torch.from_numpy(frames).cuda()
    for name in sorted(ir.KERNELS):
        want = reference(orc, "rgb", frames, spec, name, 256, ("variants",))
        compare(be.idiff(dev, P, *ir.KERNELS[name], 256).cpu().numpy(), want, name)
    del P


def test_image_ditherer_paths_with_the_instance(gpu, orc):
    import torch
    from PIL import Image
    import metric_ref as mr
    be, dl = gpu
    from dither_pie_amd import video_processor as vp
    rs = np.random.RandomState(31)
    arr = rs.randint(0, 256, (17, 33, 3)).astype(np.uint8)              # a 33 x 17 image
    arr[:, :, 1] = np.linspace(0, 255, 33).astype(np.uint8)[None, :]
    img = Image.fromarray(arr, "RGB")
    pal = palette_of(16)
    spec = dl.prepare_palette(pal, False)
    s = dl.IntegerErrorDiffusionDitherStrategy("jjn")
    results = {}
    for metric in METRICS:
        d = dl.ImageDitherer(num_colors=16, dither_mode=s, palette=pal, metric=metric)
        want = ir.idiff_u8(adapter(orc, metric), arr, *spec, *ir.KERNELS["jjn"], 256)
        got = d.apply_dithering(img)
        assert got.mode == "RGB" and got.size == (33, 17) and np.array_equal(np.asarray(got), want), metric
        planes, colours = d.apply_dithering_frames_indexed(torch.from_numpy(arr).cuda())
        assert planes.shape == (17, 33) and np.array_equal(colours[planes.cpu().numpy()], want), metric
        png = d.apply_dithering_png(img)
        dec = Image.open(io.BytesIO(png))
        assert dec.mode == "P" and np.array_equal(np.asarray(dec.convert("RGB")), want), metric
        stack = np.stack([arr, arr[::-1].copy()])
        rgb = vp.process_frames(torch.from_numpy(stack).cuda(), d)
        assert np.array_equal(rgb[0].cpu().numpy(), want) and not np.array_equal(rgb[1].cpu().numpy(), want), metric
        results[metric] = want
        assert d.dither_mode is s                                       # the hook stores nothing and replaces nothing
    assert not np.array_equal(results["rgb"], results["oklab"])         # the metric changes the picture
    from dither_pie_amd import sharding
    with pytest.raises(ValueError):                                     # errors cross band edges: no row-band sharding
        sharding.dither_band(d, torch.from_numpy(arr[:8].copy()).cuda(), 0)
