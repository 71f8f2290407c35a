"""GPU tier of the clip-wide palettes: dp_distinct_stream_add_u8 against dp_distinct_first_u8 over the concatenated buffers,
dp_hist_sample_u8 against the numpy restatement (tests/clip_palette_ref.py), clip_palette.ClipPalette (median cut against the
reference's palettes of tests/golden/clip.json, k-means against Lloyd over the resident pixels), the wrappers of ColorReducer
and VideoProcessor.scan_palette through the ffmpeg stand-ins of the pipe tests."""
import json
import os
import stat
import sys

import numpy as np
import pytest

import clip_palette_ref as cr
from clip_spec import clip_frames
from conftest import GOLDEN, fake_ffmpeg_tools

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    return torch


@pytest.fixture(scope="module")
def be(T):
    from dither_pie_amd import backend
    return backend


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _odd(T, a):
    """The pixels on the device at an ODD byte address (a view one byte into a fresh buffer)."""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 3)
    buf = T.empty(a.size + 1, dtype=T.uint8, device="cuda")
    v = buf[1:].view(-1, 3)
    v.copy_(T.from_numpy(a))
    assert v.data_ptr() % 2 == 1
    return v


def _check_stream(T, be, s, bufs, odd=False):
    """Feed bufs into the stream s; after every add the list is distinct_first of everything fed so far (device kernel and
    numpy restatement), list and count exactly."""
    fed = []
    for b in bufs:
        b = np.asarray(b, np.uint8).reshape(-1, 3)
        s.add(_odd(T, b) if odd else _dev(T, b))
        fed.append(b)
        allpx = np.concatenate(fed)
        got = s.colours().cpu().numpy()
        assert len(s) == len(got)
        if len(allpx):
            want = be.distinct_first(_dev(T, allpx)).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (len(fed), got.shape, want.shape)
            assert np.array_equal(got, cr.distinct_first(allpx))
        else:
            assert len(got) == 0


def test_stream_distinct_equals_distinct_first_of_the_concatenation(T, be):
    rs = np.random.RandomState(1)
    s = be.DistinctStream()
    assert len(s) == 0 and s.colours().shape == (0, 3)
    _check_stream(T, be, s, [[[7, 8, 9]]])                                                   # one pixel
    s.reset()
    a = rs.randint(0, 256, (500, 3))
    _check_stream(T, be, s, [a, a[rs.randint(0, 500, 300)], np.zeros((0, 3))])               # a batch that appends nothing; n = 0
    s.reset()
    c = [1, 2, 3]
    _check_stream(T, be, s, [[[9, 9, 9], c, [9, 9, 9], c], [c, [4, 4, 4], c]])               # a new colour twice in a batch, again in the next
    s.reset()
    few = rs.randint(0, 64, (100000, 3))                                                     # plenty of repeats across the odd-offset batches
    at, bufs = 0, []
    for n in (1, 3, 63, 64, 65, 4097):
        bufs.append(few[at:at + n])
        at += n
    _check_stream(T, be, s, bufs, odd=True)
    s.reset()
    eight = rs.randint(0, 256, (8, 3))                                                       # a few-colour clip: 8 colours over 3 batches
    _check_stream(T, be, s, [eight[rs.randint(0, 3, 5000)], eight[rs.randint(0, 6, 5000)], eight[rs.randint(0, 8, 5000)]])
    assert len(s) == 8


def test_stream_distinct_across_compaction_blocks_and_after_reset(T, be):
    px = np.random.RandomState(2).randint(0, 256, (300007, 3))
    s = be.DistinctStream()
    s.add(_dev(T, np.random.RandomState(3).randint(0, 256, (999, 3)).astype(np.uint8)))      # state to be forgotten
    s.reset()
    assert len(s) == 0
    before = 0
    for part in (px[:1], px[1:70001], px[70001:]):
        s.add(_dev(T, part.astype(np.uint8)))
        if len(part) > 200000:
            assert len(s) - before > 65536                                                   # > 65 536 new colours in one call
        before = len(s)
    want = be.distinct_first(_dev(T, px.astype(np.uint8))).cpu().numpy()
    got = s.colours().cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, cr.distinct_first(px))


FIVE = [["rnd", 32, 40, 21], ["imgl", 32, 40, 22, "smooth"], ["flat", 32, 40, [3, 3, 3]], ["imgl", 32, 40, 23, "dark"], ["grad", 32, 40]]


def _clip(T, frames, groups, **kw):
    from dither_pie_amd.clip_palette import ClipPalette
    c = ClipPalette(**kw)
    at = 0
    for g in groups:
        c.add(_dev(T, np.stack(frames[at:at + g])))
        at += g
    assert at == len(frames)
    return c


def test_batching_invariance(T):
    frames = clip_frames(FIVE)
    ref = None
    for groups in ((5,), (1, 4), (2, 3), (1, 1, 1, 1, 1)):
        c = _clip(T, frames, groups)
        got = (c.colours().cpu().numpy(), c.median_cut(16), c.median_cut(256), c.n_pixels, c.n_distinct)
        assert got[3] == 5 * 32 * 40 and got[4] == len(got[0])
        if ref is None:
            ref = got
            assert np.array_equal(got[0], cr.distinct_first(np.concatenate([f.reshape(-1, 3) for f in frames])))
        else:
            assert np.array_equal(ref[0], got[0]) and ref[1:] == got[1:], groups


def test_median_cut_equals_the_reference_fixtures(T):
    from dither_pie_amd.clip_palette import ClipPalette
    with open(os.path.join(GOLDEN, "clip.json")) as f:
        spec = json.load(f)
    for name, c in spec["clips"].items():
        clip = ClipPalette(use_gamma=c["use_gamma"])
        for fr in clip_frames(c["frames"]):                       # frames of differing geometry: one add each
            clip.add(_dev(T, fr))
        assert clip.n_pixels == c["n_pixels"]
        for n, want in c["palettes"].items():
            assert clip.median_cut(int(n)) == [tuple(p) for p in want], (name, n)


def test_median_cut_equals_reduce_colors_of_the_stack(T):
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    from oracle.oracle import imgl, rnd
    frames = np.stack([imgl(270, 480, 31, "smooth"), rnd(270, 480, 32), imgl(270, 480, 33, "dark")])
    stack = frames.reshape(3 * 270, 480, 3)
    assert stack.shape[0] * stack.shape[1] >= 100000              # reduce_colors takes the device path for the stack
    for n in (16, 256):
        assert ColorReducer.reduce_colors_frames(_dev(T, frames), n) == ColorReducer.reduce_colors(Image.fromarray(stack), n)


def _rank_cases(px, rs):
    px = np.asarray(px, np.uint8).reshape(-1, 3)
    hist = cr.histogram(px)
    total = len(px)
    ends = np.cumsum(hist)
    ranks = [0, total - 1, 0, total - 1, total // 2, total // 2]                             # both ends, duplicates
    slot = int(np.argmax(hist))                                                              # a run with count > 1 where there is one
    ranks += [int(ends[slot] - hist[slot]), int(ends[slot] - 1)]
    cell_ends = np.cumsum(hist.reshape(4096, 4096).sum(axis=1))
    occupied = np.nonzero(hist.reshape(4096, 4096).sum(axis=1))[0]
    for cell in occupied[[0, len(occupied) // 2, -1]]:                                       # either side of a cell boundary
        ranks += [int(cell_ends[cell] - 1), int(min(cell_ends[cell], total - 1))]
    gaps = np.diff(occupied)
    if len(gaps):                                                                            # the rank after the longest run of empty cells
        cell = occupied[int(np.argmax(gaps)) + 1]
        ranks += [int(cell_ends[cell - 1]), int(max(cell_ends[cell - 1] - 1, 0))]
    ranks += rs.randint(0, total, 200).tolist()
    return hist, np.array(ranks, np.int64)


def test_rank_sample_equals_the_restatement(T, be):
    from oracle.oracle import imgl, rnd
    rs = np.random.RandomState(5)
    flat = np.empty((64, 64, 3), np.uint8)
    flat[:] = (200, 17, 99)
    noise = [rnd(64, 64, 41 + i) for i in range(3)]
    big = np.concatenate([imgl(200, 300, 44, "smooth").reshape(-1, 3), rnd(100, 100, 45).reshape(-1, 3)])
    assert len(big) == 70000
    for name, batches in (("flat", [flat]), ("noise", noise), ("70000", [big[:1], big[1:30001], big[30001:]])):
        h = be.ColourHistogram(device="cuda")
        for i, b in enumerate(batches):
            h.add(_dev(T, b).view(-1, 3), accumulate=i > 0)
        px = np.concatenate([np.asarray(b).reshape(-1, 3) for b in batches])
        hist, ranks = _rank_cases(px, rs)
        want, bad = cr.rank_sample(hist, ranks)
        assert bad == 0
        assert np.array_equal(h.sample(ranks).cpu().numpy(), want), name
        assert np.array_equal(h.sample(T.from_numpy(ranks).cuda()).cpu().numpy(), want), name
        for r in (-1, len(px), 1 << 40):
            with pytest.raises(ValueError, match="ranks lie outside"):
                h.sample(np.array([0, r], np.int64))
        assert h.sample(np.zeros(0, np.int64)).shape == (0, 3)
    with pytest.raises(ValueError):
        h.sample(np.zeros(be.HIST_SAMPLE_MAX_RANKS + 1, np.int64))


KM = [["imgl", 64, 64, 51, "smooth"], ["rnd", 64, 64, 52], ["imgl", 64, 64, 53, "dark"], ["grad", 64, 64]]


def test_kmeans_is_lloyd_over_the_concatenated_pixels(T, be):
    from dither_pie_amd import kmeans
    frames = clip_frames(KM)
    px = np.concatenate([f.reshape(-1, 3) for f in frames])
    assert len(px) > kmeans.SAMPLE
    clip = _clip(T, frames, (1, 3))
    hist = cr.histogram(px)
    for K in (8, 32):
        ranks = clip.seed_ranks(42)
        assert np.array_equal(ranks, np.random.RandomState(42).randint(0, len(px), kmeans.SAMPLE))
        sample = clip._hist.sample(ranks)
        assert np.array_equal(sample.cpu().numpy(), cr.rank_sample(hist, ranks)[0])          # the sample is the restatement's
        init = kmeans.kmeans_plusplus_device(sample, K, np.random.RandomState(42))
        centres, inertia, n_iter = kmeans.lloyd(_dev(T, px), init, histogram=False, centres_are_data_points=True)
        pal, got_c, got_i, got_n = clip.kmeans_fit(K)
        assert got_n == n_iter and np.array_equal(got_c, centres)                           # integer totals: exact
        assert abs(got_i - inertia) <= 1e-9 * abs(inertia)                                  # (a float64 sum over K terms)
        assert pal == [tuple(int(v) for v in c) for c in centres.astype(int)] == clip.kmeans(K)
        # a pure function of the multiset: shuffled frame order, other batching, pixels shuffled within the clip
        assert _clip(T, frames[::-1], (2, 2)).kmeans(K) == pal
        shuffled = px[np.random.RandomState(6).permutation(len(px))].reshape(4, 64, 64, 3)
        assert _clip(T, list(shuffled), (4,)).kmeans(K) == pal
    small = _clip(T, [f[:20, :30] for f in frames], (4,))                                    # <= 10 000 pixels: every pixel seeds
    assert np.array_equal(small.seed_ranks(), np.arange(4 * 600))
    assert len(small.kmeans(5)) == 5
    with pytest.raises(ValueError):
        clip.kmeans(257)
    from dither_pie_amd.clip_palette import ClipPalette
    for fit in (lambda c: c.kmeans(4), lambda c: c.median_cut(4)):
        with pytest.raises(ValueError, match="no pixels"):
            fit(ClipPalette())
    assert len(clip.add(_dev(T, frames[0])).kmeans(8)) == 8                                  # a fit does not consume the accumulator


def test_clip_palette_beats_the_first_frame_palette_on_a_dark_opening(T):
    """A clip of one flat dark frame and two colourful ones, quantised without dithering: the palette the first frame gives
    knows one colour; a palette fitted to the clip has strictly less squared error over the clip, from either source."""
    from dither_pie_amd.dithering_lib import ColorReducer, DitherMode, ImageDitherer
    from oracle.oracle import imgl, rnd
    dark = np.empty((48, 64, 3), np.uint8)
    dark[:] = (6, 5, 7)
    frames = _dev(T, np.stack([dark, imgl(48, 64, 61, "smooth"), rnd(48, 64, 62)]))

    def sse(palette):
        d = ImageDitherer(16, DitherMode.NONE, palette)
        out = d.apply_dithering_frames(frames)
        return int(((out.to(T.int64) - frames.to(T.int64)) ** 2).sum().item()), d.palette

    first_sse, first_pal = sse(None)
    assert set(first_pal) <= {(6, 5, 7), (0, 0, 0)}                   # what the first frame knows
    for pal in (ColorReducer.reduce_colors_frames(frames, 16), ColorReducer.generate_kmeans_palette_frames(frames, 16)):
        assert len(pal) == 16
        assert sse(list(pal))[0] < first_sse


def test_every_counts_across_add_calls(T):
    from dither_pie_amd.clip_palette import ClipPalette
    frames = clip_frames(FIVE)
    a = ClipPalette().add(_dev(T, np.stack(frames[:3])), every=2).add(_dev(T, np.stack(frames[3:])), every=2)
    b = ClipPalette().add(_dev(T, np.stack([frames[0], frames[2], frames[4]])))
    assert a.n_frames == 3 and a.n_pixels == b.n_pixels == 3 * 32 * 40
    assert np.array_equal(a.colours().cpu().numpy(), b.colours().cpu().numpy())
    assert a.median_cut(16) == b.median_cut(16) and a.kmeans(8) == b.kmeans(8)
    one_by_one = ClipPalette()
    for f in frames:
        one_by_one.add(_dev(T, f), every=2)                           # [H,W,3] frames, one call each
    assert one_by_one.n_frames == 3 and one_by_one.median_cut(16) == b.median_cut(16)
    g = ClipPalette(use_gamma=True).add(_dev(T, frames[1]))
    from dither_pie_amd import _tables
    assert np.array_equal(g.colours().cpu().numpy(), cr.distinct_first(_tables.LUT_IN[frames[1]]))


def test_scan_palette_through_the_decoder_stand_in(T, tmp_path, monkeypatch):
    from dither_pie_amd.clip_palette import ClipPalette
    from dither_pie_amd.video_processor import VideoProcessor
    from oracle.oracle import imgl, rnd
    frames = np.stack([imgl(48, 64, 70 + i, "smooth") if i % 2 else rnd(48, 64, 70 + i) for i in range(11)])
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    seen = []
    vp = VideoProcessor(progress_callback=lambda frac, msg: seen.append((frac, msg)), devices=[0])
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", 4 * 48 * 64 * 3)      # batches of 4 frames: 4 + 4 + 3
    direct = ClipPalette().add(_dev(T, frames))
    assert vp.scan_palette("in.mp4", "median_cut", 16) == direct.median_cut(16)
    assert vp.last_scan_stats["frames"] == 11 and vp.last_scan_stats["batch_frames"] == 4
    assert seen[0][0] == 0.0 and seen[-1][0] == 1.0 and [f for f, _ in seen] == sorted(f for f, _ in seen)
    assert any(m.startswith("Scanned 11/") for _, m in seen)
    assert vp.scan_palette("in.mp4", "kmeans", 8, random_state=7) == direct.kmeans(8, random_state=7)
    every3 = ClipPalette(use_gamma=True).add(_dev(T, frames[:9]), every=3)
    assert vp.scan_palette("in.mp4", "median_cut", 16, every=3, max_frames=9, use_gamma=True) == every3.median_cut(16)
    assert vp.last_scan_stats["frames"] == 9
    with pytest.raises(ValueError):
        vp.scan_palette("in.mp4", "octree", 16)


def test_scan_palette_fails_as_the_pipes_path_does(T, tmp_path, monkeypatch):
    from dither_pie_amd.video_processor import VideoProcessor
    from oracle.oracle import rnd
    frames = np.stack([rnd(48, 64, 80 + i) for i in range(6)])
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames, trailing=b"\x01\x02\x03")   # a stream that ends inside a frame
    vp = VideoProcessor(devices=[0])
    with pytest.raises(RuntimeError, match="not a whole number"):
        vp.scan_palette("in.mp4", "median_cut", 16)
    # a decoder that dies mid-stream: three whole frames, then exit status 1
    raw = tmp_path / "input.raw"
    ff = tmp_path / "ffmpeg"
    ff.write_text(f"#!{sys.executable}\nimport sys\nsys.stdout.buffer.write(open({str(raw)!r}, 'rb').read()[:{3 * 48 * 64 * 3}])\n"
                  "sys.stdout.flush()\nsys.exit(1)\n")
    ff.chmod(ff.stat().st_mode | stat.S_IXUSR)
    with pytest.raises(RuntimeError, match=r"ffmpeg failed \(decoder 1\)"):
        vp.scan_palette("in.mp4", "kmeans", 8)
