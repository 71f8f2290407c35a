"""GPU tier of Oklab palette fitting (include/ditherpie_hip_okfit.h): the kernels against the host statement (dp_okfit_host) and
the numpy statement (tests/okfit_ref.py), bit for bit -- palette, centres, n_iter and distortion -- on the cases the CPU tier
holds the host statement to, at point counts on the edges of the kernels' tiles and at centre counts on the edges of theirs;
the compaction of a colour histogram into point records; ClipPalette.oklab, ColorReducer.generate_oklab_palette_frames, the video
scans with source="oklab" and ImageDitherer(palette_fit="oklab") end to end.

The fit kernels' tile: a workgroup of 256 lanes (okfit.hip: kFitBlock) takes 256 points per stride step, a wave 64 of them, and
a launch has at most 512 workgroups (kFitMaxBlocks) -- so 63 / 64 / 65 sit on a wave's edge, 255 / 256 / 257 on a workgroup's,
4097 is 16 workgroups and one point, and 512 * 256 + 1 = 131 073 is the first size at which a lane strides to a second point."""
import numpy as np
import pytest

import metric_ref as mr
import okfit_ref as ok
from conftest import fake_ffmpeg_tools

pytestmark = pytest.mark.gpu

FIT_BLOCK, FIT_MAX_BLOCKS = 256, 512
CASES = ok.cases()


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    from dither_pie_amd import dithering_lib as dl
    yield backend, dl
    torch.cuda.synchronize()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3])


def three_way(be, codes, counts, K, max_iter=100):
    """kernel = host statement = numpy statement"""
    want = ok.fit_points(codes, counts, K, max_iter)
    host = be.okfit_host(codes, counts, K, max_iter)
    got = be.okfit(be.okfit_points(codes, counts), K, max_iter)
    assert got[0].dtype == np.uint8 and got[0].shape == (K, 3) and got[1].dtype == np.int32 and got[1].shape == (K, 3)
    assert same(host, want), ("host", host[2:], want[2:])
    assert same(got, want), ("kernel", got[2:], want[2:], np.nonzero((got[1] != want[1]).any(1))[0][:8], np.nonzero((got[0] != want[0]).any(1))[0][:8])
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_statements_on_the_cpu_cases(gpu, name):
    be, _ = gpu
    three_way(be, *CASES[name])


@pytest.mark.parametrize("n, K, max_iter", [(63, 16, 100), (64, 16, 100), (65, 16, 100), (255, 16, 100), (256, 16, 100), (257, 16, 100), (4097, 16, 100),
                                            (FIT_BLOCK * FIT_MAX_BLOCKS + 1, 16, 2)])
def test_point_counts_on_wave_workgroup_and_stride_edges(gpu, n, K, max_iter):
    be, _ = gpu
    codes, counts = ok.random_points(n, 500 + n % 1000)
    res = three_way(be, codes, counts, K, max_iter)
    print(n, "points:", res[2], "passes")


@pytest.mark.parametrize("K", [1, 16, 17, 64, 65, 256])
def test_centre_counts(gpu, K):
    be, _ = gpu
    codes, counts = ok.random_points(1000, 600 + K)
    three_way(be, codes, counts, K)


def test_points_kernel_writes_the_records_of_the_statement(gpu):
    be, _ = gpu
    codes, counts = ok.random_points(777, 9, max_count=(1 << 32) // 1000)
    c, k, lab = be.okfit_points_numpy(be.okfit_points(codes, counts))
    assert np.array_equal(c, codes) and np.array_equal(k, counts) and np.array_equal(lab, mr.lab(ok.colours_of(codes)))
    assert lab.dtype == np.int16


# ---------------------------------------------------------------------------------------------------- histograms
def frames_for_histograms():
    rs = np.random.RandomState(70)
    noise = rs.randint(0, 256, (48, 64, 3)).astype(np.uint8)             # a 64 x 48 frame
    two = np.zeros((48, 64, 3), np.uint8)
    two[:] = (200, 30, 30)
    two[10:20, 5:50] = (10, 20, 250)
    return noise, two


@pytest.mark.parametrize("which, K", [(0, 16), (0, 4), (1, 2), (1, 16)])
def test_frames_through_the_colour_histogram(gpu, which, K):
    import torch
    be, _ = gpu
    frame = frames_for_histograms()[which]
    hist = be.ColourHistogram(torch.from_numpy(frame).cuda().view(-1, 3))
    codes, counts = ok.points_of(frame)
    want = ok.fit_points(codes, counts, K)
    assert same(be.okfit(hist, K), want)
    assert same(be.okfit(hist.points(), K), want) and same(be.okfit_host(codes, counts, K), want)
    if which == 1:
        assert len(codes) == 2 and hist.n_occupied() == 2
        assert {tuple(c) for c in want[0].tolist()} == {(200, 30, 30), (10, 20, 250)} and want[3] == 0


def test_compaction_is_the_sorted_unique_of_the_pixels(gpu):
    import torch
    be, _ = gpu
    rs = np.random.RandomState(71)
    parts = [rs.randint(0, 256, (m, 3)).astype(np.uint8) for m in (3000, 1, 4500)]
    parts[2][:2000] = parts[0][:2000]                                   # colours that come back in a later add
    parts[2][2000:3000] = parts[2][2000:3000] // 16 * 16                # whole runs of the table with one occupied colour
    parts[0][:5] = [(0, 0, 0), (255, 255, 255), (0, 0, 255), (255, 0, 0), (15, 15, 15)]   # the corners of the cube, the end of a cell
    hist = be.ColourHistogram(device="cuda")
    assert hist.n_occupied() == 0 and hist.points().shape == (0, 16)
    seen = []
    for i, p in enumerate(parts):                                       # a histogram accumulated over three add calls
        hist.add(torch.from_numpy(p).cuda(), accumulate=i > 0)
        seen.append(p)
        codes, counts = ok.points_of(np.concatenate(seen))
        n = len(codes)
        assert hist.n_occupied() == n
        c, k, lab = be.okfit_points_numpy(hist.points())
        assert np.array_equal(c, codes) and np.array_equal(k, counts) and np.array_equal(lab, mr.lab(ok.colours_of(codes))), i
    # a capacity one short of n: the true n is reported, nothing past the capacity is written (the tensor has no room for it:
    # tests/test_gpu_okfit_memory.py looks at the bytes behind it), and the call succeeds
    pts, n_true = hist.points(capacity=n - 1)
    assert n_true == n and pts.shape == (n - 1, 16)
    c, k, _ = be.okfit_points_numpy(pts)
    assert np.array_equal(c, codes[:-1]) and np.array_equal(k, counts[:-1])
    pts, n_true = hist.points(capacity=n + 3)
    assert n_true == n and pts.shape == (n, 16)
    pts, n_true = hist.points(capacity=0)
    assert n_true == n and pts.shape == (0, 16)


# ---------------------------------------------------------------------------------------------------- clips
def clip_frames():
    rs = np.random.RandomState(72)
    f = rs.randint(0, 256, (6, 12, 16, 3)).astype(np.uint8)
    f[3:] = f[3:] // 4 * 4                                              # frames that share colours
    return f


def test_clip_fit_is_independent_of_batching_and_frame_order(gpu):
    import torch
    from dither_pie_amd.clip_palette import ClipPalette
    be, dl = gpu
    frames = clip_frames()
    dev = torch.from_numpy(frames).cuda()
    want = ok.fit(frames, 16)                                           # the statement on the stacked frames
    want_list = [tuple(int(v) for v in c) for c in want[0]]
    whole = ClipPalette().add(dev)
    pal, centres, n_iter, dist = whole.oklab_fit(16)
    assert pal == want_list and same((np.array(pal, np.uint8), centres, n_iter, dist), want)
    assert whole.oklab(16) == want_list                                 # a fit does not consume the accumulator
    one_by_one = ClipPalette()
    for i in (4, 0, 5, 2, 1, 3):                                        # another frame order, one add per frame
        one_by_one.add(dev[i])
    assert one_by_one.oklab(16) == want_list
    split = ClipPalette().add(dev[:1]).add(dev[1:4]).add(dev[4:])
    assert split.oklab(16) == want_list
    assert dl.ColorReducer.generate_oklab_palette_frames(dev, 16) == want_list
    every = dl.ColorReducer.generate_oklab_palette_frames(dev, 8, every=2, max_iter=3)
    assert every == ClipPalette().add(dev, every=2).oklab(8, max_iter=3) == [tuple(int(v) for v in c) for c in ok.fit(frames[::2], 8, 3)[0]]
    from PIL import Image
    assert dl.ColorReducer.generate_oklab_palette(Image.fromarray(frames[0], "RGB"), 5) == [tuple(int(v) for v in c) for c in ok.fit(frames[0], 5)[0]]
    with pytest.raises(ValueError, match="no pixels"):
        ClipPalette().oklab(4)
    with pytest.raises(ValueError, match="256 colours"):
        whole.oklab(257)
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        ClipPalette(use_gamma=True).add(dev).oklab(4)
    assert whole.kmeans(4) and whole.median_cut(4)                      # the other producers still read the same accumulator


# ---------------------------------------------------------------------------------------------------- video scans
def scene_frames():
    """12 frames of 8 x 8: six whose colours lie in one 16^3 cell of the cube, six in another -- one cut, at frame 6."""
    rs = np.random.RandomState(73)
    a = rs.randint(32, 48, (6, 8, 8, 3))
    b = rs.randint(16, 32, (6, 8, 8, 3)) + np.array([144, 48, 192])
    return np.concatenate([a, b]).astype(np.uint8)


def test_video_scans_with_the_oklab_source(gpu, tmp_path, monkeypatch):
    import torch
    from dither_pie_amd.clip_palette import ClipPalette
    from dither_pie_amd.video_processor import VideoProcessor
    frames = scene_frames()
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", 4 * 8 * 8 * 3)   # batches of 4: the cut falls inside one
    vp = VideoProcessor(devices=[0])
    fresh = lambda lo, hi, n, every=1: ClipPalette().add(torch.from_numpy(frames[lo:hi]).cuda(), every=every).oklab(n)   # noqa: E731
    assert vp.scan_palette("in.mp4", "oklab", 8) == fresh(0, 12, 8)
    assert vp.scan_palette("in.mp4", "oklab", 8) == [tuple(int(v) for v in c) for c in ok.fit(frames, 8)[0]]
    assert vp.scan_palette("in.mp4", "oklab", 4, every=3, max_frames=10) == fresh(0, 10, 4, 3)
    scenes = vp.scan_scenes("in.mp4", "oklab", 8, min_scene_frames=3)
    assert [(s.start, s.end) for s in scenes] == [(0, 6), (6, 12)]
    for s in scenes:
        assert s.palette == fresh(s.start, s.end, 8), s.start
    assert scenes[0].palette != scenes[1].palette and vp.last_scan_stats["skipped"] == 0


# ---------------------------------------------------------------------------------------------------- ImageDitherer
def test_image_ditherer_fits_its_palette_in_oklab(gpu):
    from PIL import Image
    be, dl = gpu
    img = np.random.RandomState(74).randint(0, 256, (32, 32, 3)).astype(np.uint8)
    want_pal = ok.fit(img, 16)[0]
    d = dl.ImageDitherer(num_colors=16, dither_mode=dl.DitherMode.BAYER, palette=None, dither_params={"size": "4x4"}, palette_fit="oklab", metric="oklab")
    got = np.asarray(d.apply_dithering(Image.fromarray(img, "RGB")))
    assert d.palette == [tuple(int(v) for v in c) for c in want_pal]     # the kept palette is the statement's
    bayer4 = dl.DitherUtils.get_threshold_matrix(dl.DitherMode.BAYER, "4x4")
    assert np.array_equal(got, mr.ordered_u8(img, want_pal.astype(np.float32), want_pal, bayer4))
    # independent of the metric: the same palette under the RGB search, and today's median cut without the keyword
    rgb = dl.ImageDitherer(num_colors=16, dither_mode=dl.DitherMode.NONE, palette=None, palette_fit="oklab")
    rgb.apply_dithering(Image.fromarray(img, "RGB"))
    assert rgb.palette == d.palette
    plain = dl.ImageDitherer(num_colors=16, dither_mode=dl.DitherMode.NONE, palette=None, metric="oklab")
    plain.apply_dithering(Image.fromarray(img, "RGB"))
    assert plain.palette == dl.ColorReducer.reduce_colors(Image.fromarray(img, "RGB"), 16) != d.palette
