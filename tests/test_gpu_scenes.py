"""GPU tier of the per-scene palettes, on the product library: dp_frame_signatures_u8 and dp_signature_distances against the
numpy restatement (tests/scene_ref.py) over frame sizes, batch sizes, base alignments and contents; backend.SceneStream over
splits of a stream; ClipPalette.reset(); VideoProcessor.scan_scenes through the ffmpeg stand-ins of the pipe tests on the
synthetic three-scene clip; process_video_streaming(scene_palettes=...) against process_frames run scene by scene."""
import numpy as np
import pytest

import scene_ref as sr
from conftest import fake_ffmpeg_tools

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (3, 5), (17, 33), (64, 64), (129, 257), (300, 400)]   # 300 x 400: several workgroups share a frame's bins


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


@pytest.fixture(scope="module")
def clip():
    frames, moved = sr.three_scene_clip()
    return frames, moved, sr.signatures(frames)


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _at_offset(T, frames, off):
    """The frames on the device at a base address = off (mod 4): a slice of a byte buffer."""
    frames = np.ascontiguousarray(frames, np.uint8)
    buf = T.empty(frames.size + 4, dtype=T.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    v = buf[off:off + frames.size].view(frames.shape)
    v.copy_(T.from_numpy(frames))
    assert v.data_ptr() % 4 == off
    return v


def _sig(be, x):
    s = be.frame_signatures(x)
    assert s.dtype.is_signed and s.shape == (x.shape[0] if x.dim() == 4 else 1, 4096)
    return s.cpu().numpy().astype(np.int64)


def _contents(rs, n, h, w):
    noise = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    flat = np.empty((n, h, w, 3), np.uint8)
    flat[:] = (200, 17, 99)
    borders = np.array([15, 16, 239, 240, 255], np.uint8)[rs.randint(0, 5, (n, h, w, 3))]   # colours on cell borders
    return {"noise": noise, "flat": flat, "borders": borders}


@pytest.mark.parametrize("h, w", SIZES)
def test_signatures_over_sizes_batches_alignments_and_contents(T, be, h, w):
    rs = np.random.RandomState(h * 1000 + w)
    for n in (1, 2, 3, 17):
        for name, frames in _contents(rs, n, h, w).items():
            want = sr.signatures(frames)
            if name == "flat":
                assert (want[:, (200 >> 4) << 8 | (17 >> 4) << 4 | (99 >> 4)] == h * w).all()   # all counts land in one bin
            offsets = (0, 1, 2, 3) if (n in (1, 3) or name == "noise") else (0, 3)
            for off in offsets:
                assert np.array_equal(_sig(be, _at_offset(T, frames, off)), want), (n, name, off)
    one = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    assert np.array_equal(_sig(be, _dev(T, one)), sr.signatures(one))    # [H,W,3]
    assert be.frame_signatures(T.empty((0, h, w, 3), dtype=T.uint8, device="cuda")).shape == (0, 4096)


def test_a_prefilled_signature_buffer_comes_out_exact(T, be):
    from dither_pie_amd import _lib
    L = _lib.load()
    frames = np.random.RandomState(3).randint(0, 256, (3, 17, 33, 3)).astype(np.uint8)
    x = _dev(T, frames)
    sig = T.full((3, 4096), -1, dtype=T.int32, device="cuda")            # 0xFF everywhere: the zeroing is part of the call
    assert L.dp_frame_signatures_u8(x.data_ptr(), 3, 17, 33, sig.data_ptr(), be._stream()) == 0, L.dp_last_error()
    assert np.array_equal(sig.cpu().numpy().astype(np.int64), sr.signatures(frames))


def test_distances_are_exact(T, be, clip):
    frames, moved, sig = clip
    h, w = sr.H, sr.W
    s = be.SceneStream()
    same = np.stack([frames[0], frames[0], frames[1]])                   # identical, then a permutation: 0, 0, 0
    assert s.add(_dev(T, same)).tolist() == [0, 0, 0]
    s.reset()
    disjoint = np.stack([frames[0], frames[16], frames[39], frames[1]])  # frames of three scenes: no cell shared
    assert s.add(_dev(T, disjoint)).tolist() == [0, 2 * h * w, 2 * h * w, 2 * h * w]
    s.reset()
    m = moved[0]
    assert s.add(_dev(T, frames[m - 1:m + 2])).tolist() == [0, 2 * sr.MOVED, 2 * sr.MOVED]   # m pixels moved to another cell: 2 m
    s.reset()
    d = s.add(_dev(T, frames))
    assert d.dtype == T.int64 and d.is_cuda and np.array_equal(d.cpu().numpy(), sr.distances(sig))
    big = np.zeros((2, 300, 400, 3), np.uint8)                           # the largest distance of a frame size: 2 h w
    big[1] = 255
    assert be.SceneStream().add(_dev(T, big)).tolist() == [0, 2 * 300 * 400]


def test_scene_stream_carries_the_last_signature(T, be, clip):
    frames, _, sig = clip
    frames, want = frames[10:27], sr.distances(sig[10:27])               # 17 frames across both cuts
    x = _dev(T, frames)
    s = be.SceneStream()
    for sizes in ((17,), (1, 16), (8, 9), (1,) * 17):
        s.reset()
        got, at = [], 0
        for n in sizes:
            got += s.add(x[at:at + n]).tolist()
            at += n
        assert got == want.tolist(), sizes
    assert s.add(x[:3]).tolist()[0] == int(np.abs(sig[10] - sig[26]).sum())   # without a reset the stream goes on
    assert s.reset().add(x[16:17]).tolist() == [0]                       # reset(): the next first distance is 0
    assert s.add(x[:0]).shape == (0,)
    with pytest.raises(ValueError, match="reset"):
        s.add(_dev(T, np.zeros((1, 8, 8, 3), np.uint8)))                 # another h * w without a reset
    s.reset()
    assert s.add(_dev(T, np.zeros((2, 8, 8, 3), np.uint8))).tolist() == [0, 0]
    with pytest.raises(TypeError):
        s.add(frames)


def test_clip_palette_reset_makes_a_fresh_object(T):
    from dither_pie_amd.clip_palette import ClipPalette
    from oracle.oracle import imgl, rnd
    a = np.stack([rnd(32, 40, 91), imgl(32, 40, 92, "smooth"), rnd(32, 40, 93)])
    b = np.stack([imgl(32, 40, 94, "dark"), rnd(32, 40, 95), imgl(32, 40, 96, "smooth"), rnd(32, 40, 97)])
    for gamma in (False, True):
        used = ClipPalette(use_gamma=gamma).add(_dev(T, a), every=2)
        assert used.n_frames == 2 and used.reset() is used
        assert (used.n_pixels, used.n_frames, used.n_distinct) == (0, 0, 0)
        with pytest.raises(ValueError, match="no pixels"):
            used.median_cut(16)
        used.add(_dev(T, b[:1]), every=3).add(_dev(T, b[1:]), every=3)    # `every` counts from the first frame after the reset
        fresh = ClipPalette(use_gamma=gamma).add(_dev(T, b), every=3)
        assert (used.n_pixels, used.n_frames) == (fresh.n_pixels, fresh.n_frames) == (2 * 32 * 40, 2)
        assert np.array_equal(used.colours().cpu().numpy(), fresh.colours().cpu().numpy())
        assert used.median_cut(16) == fresh.median_cut(16) and used.kmeans(8) == fresh.kmeans(8)
        assert T.equal(used._hist.buf[:1 << 26], fresh._hist.buf[:1 << 26])   # the whole count table, not only what the fits read


# ---------------------------------------------------------------------------------------------------- scan_scenes
def _fresh_palette(T, frames, lo, hi, source, n, every=1, gamma=False):
    from dither_pie_amd.clip_palette import ClipPalette
    c = ClipPalette(use_gamma=gamma).add(_dev(T, frames[lo:hi]), every=every)
    return c.median_cut(n) if source == "median_cut" else c.kmeans(n, 42)


@pytest.fixture
def scanner(T, clip, tmp_path, monkeypatch):
    from dither_pie_amd.video_processor import VideoProcessor
    frames = clip[0]
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", 4 * sr.H * sr.W * 3)   # batches of 4: the cut at 15 inside one, at 20 on an edge
    return VideoProcessor(devices=[0]), frames


def test_scan_scenes_boundaries(T, clip, scanner, monkeypatch):
    from dither_pie_amd import clip_palette
    vp, frames = scanner
    dist = sr.distances(clip[2])
    n_px = sr.H * sr.W

    def no_accumulator(*a, **k):
        raise AssertionError("source=None must not make an accumulator")
    monkeypatch.setattr(clip_palette.ClipPalette, "__init__", no_accumulator)
    for kw in (dict(min_scene_frames=3), dict(), dict(min_scene_frames=6), dict(min_scene_frames=3, max_frames=18), dict(min_scene_frames=1, threshold=0.05),
               dict(min_scene_frames=3, threshold=1.0)):
        n = kw.get("max_frames", 40)
        want = sr.scene_ranges(n, sr.cut_starts(dist[:n], n_px, kw.get("threshold", 0.4), kw.get("min_scene_frames", 8)))
        got = vp.scan_scenes("in.mp4", **kw)
        assert [(s.start, s.end) for s in got] == want and all(s.palette is None for s in got), kw
        assert vp.last_scan_stats["frames"] == n and vp.last_scan_stats["scenes"] == len(want) and vp.last_scan_stats["batch_frames"] == 4
    assert [(s.start, s.end) for s in vp.scan_scenes("in.mp4", min_scene_frames=3)] == [(0, 15), (15, 20), (20, 40)]   # no false cut at the in-scene change
    seen = []
    vp.progress_callback = lambda frac, msg: seen.append((frac, msg))
    assert [(s.start, s.end) for s in vp.scan_scenes("in.mp4")] == [(0, 15), (15, 40)]      # the default 8 is larger than the middle scene
    assert seen[0][0] == 0.0 and seen[-1][0] == 1.0 and [f for f, _ in seen] == sorted(f for f, _ in seen)


@pytest.mark.parametrize("source, n_colors", [("median_cut", 16), ("kmeans", 8)])
def test_scan_scenes_palettes_are_those_of_a_fresh_clip_palette(T, scanner, source, n_colors):
    vp, frames = scanner
    cache = {}

    def want(lo, hi, every, gamma):
        key = (lo, hi, every, gamma)
        if key not in cache:
            cache[key] = _fresh_palette(T, frames, lo, hi, source, n_colors, every, gamma)
        return cache[key]

    for kw, ranges in ((dict(min_scene_frames=3), [(0, 15), (15, 20), (20, 40)]), (dict(min_scene_frames=3, every=3), [(0, 15), (15, 20), (20, 40)]),
                       (dict(), [(0, 15), (15, 40)]), (dict(min_scene_frames=3, max_frames=18, every=3), [(0, 15), (15, 18)]),
                       (dict(min_scene_frames=3, use_gamma=True), [(0, 15), (15, 20), (20, 40)])):
        got = vp.scan_scenes("in.mp4", source, n_colors, **kw)
        assert [(s.start, s.end) for s in got] == ranges, kw
        for s in got:
            assert s.palette == want(s.start, s.end, kw.get("every", 1), kw.get("use_gamma", False)), (kw, s.start)
        assert vp.last_scan_stats["skipped"] == 0 and vp.last_scan_stats["signature_s"] > 0 and vp.last_scan_stats["palette_s"] > 0
    assert got[0].palette != got[1].palette                             # (the scenes share no cell: neither do their palettes)


# ---------------------------------------------------------------------------------------------------- streaming
PALETTES = [[(10, 20, 30), (70, 200, 40), (40, 90, 200), (75, 230, 250)], [(100, 0, 0), (150, 250, 250), (120, 120, 120)],
            [(180, 0, 0), (250, 250, 250), (200, 100, 50), (255, 0, 255), (181, 250, 250)]]


def _ditherer(kind):
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    if kind == "bayer":
        return ImageDitherer(16, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    return ImageDitherer(16, DitherMode.ERROR_DIFFUSION, [(0, 0, 0), (255, 255, 255)], dither_params={"variant": "floyd_steinberg"})


def _scene_by_scene(T, frames, scenes, ditherer, final=2):
    import copy
    from dither_pie_amd.video_processor import process_frames
    out = []
    for k, s in enumerate(scenes):
        d = copy.copy(ditherer)
        d.palette = list(s.palette)
        hi = len(frames) if k == len(scenes) - 1 else s.end            # frames past the last scene's end: its palette
        out.append(process_frames(_dev(T, frames[s.start:hi]), d, None, 64, final).cpu().numpy())
    return np.concatenate(out)


@pytest.fixture(scope="module")
def expected(T, clip):
    """process_frames scene by scene, once per dither mode (shared by the streaming tests)."""
    from dither_pie_amd.scenes import Scene
    scenes = [Scene(0, 15, PALETTES[0]), Scene(15, 20, PALETTES[1]), Scene(20, 36, PALETTES[2])]   # 36 ... 39 lie past the last end
    return scenes, {kind: _scene_by_scene(T, clip[0], scenes, _ditherer(kind)) for kind in ("bayer", "fs")}


@pytest.mark.parametrize("kind", ["bayer", "fs"])
@pytest.mark.parametrize("batch", [4, 5])                               # 4: the cut at 15 inside a batch, at 20 on an edge; 5: both on edges
def test_streaming_switches_palettes_at_the_scene_boundaries(T, clip, expected, tmp_path, monkeypatch, kind, batch):
    from dither_pie_amd.video_processor import VideoProcessor
    frames = clip[0]
    scenes, want = expected
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    vp = VideoProcessor(devices=[0])
    size = f"{2 * sr.W}x{2 * sr.H}".encode()
    for overlap in (True, False):
        out_path = tmp_path / f"o{int(overlap)}.bin"
        d = _ditherer(kind)
        done = vp._stream_through_pipes("in.mp4", str(out_path), d, None, 64, batch, 2, vp.get_video_info("in.mp4"), overlap=overlap,
                                        scene_palettes=scenes)
        head, body = out_path.read_bytes().split(b"\n", 1)
        assert done == 40 and head == size and body == want[kind].tobytes(), (kind, batch, overlap)
        assert d.palette == [(0, 0, 0), (255, 255, 255)]                 # the caller's ditherer keeps its own palette
    out_path = tmp_path / "api.bin"
    assert vp.process_video_streaming("in.mp4", str(out_path), _ditherer(kind), None, batch_size=batch, final_resize_multiplier=2,
                                      scene_palettes=[tuple(s) for s in scenes]) is True
    assert out_path.read_bytes().split(b"\n", 1)[1] == want[kind].tobytes()
    assert want[kind][14].tobytes() != want[kind][15].tobytes() and len(np.unique(want[kind][16].reshape(-1, 3), axis=0)) <= 3


@pytest.mark.parametrize("overlap", [True, False])
def test_streaming_with_scene_palettes_on_several_devices(T, clip, expected, tmp_path, monkeypatch, overlap):
    """Two worker streams (the one GPU named twice): batches of 2 x 4 frames, both cuts inside a batch; every piece goes
    through sharding.process_on_devices into the batch's pinned output."""
    from dither_pie_amd.video_processor import VideoProcessor
    scenes, want = expected
    fake_ffmpeg_tools(tmp_path, monkeypatch, clip[0])
    vp = VideoProcessor(devices=[0, 0])
    out_path = tmp_path / "o.bin"
    assert vp._stream_through_pipes("in.mp4", str(out_path), _ditherer("bayer"), None, 64, 4, 2, vp.get_video_info("in.mp4"), overlap=overlap,
                                    scene_palettes=scenes) == 40
    assert vp.last_pipe_stats["batch_frames"] == 8
    assert out_path.read_bytes().split(b"\n", 1)[1] == want["bayer"].tobytes()


@pytest.mark.parametrize("overlap", [True, False])
def test_a_retried_frame_keeps_its_scene_palette(T, clip, expected, tmp_path, monkeypatch, overlap):
    """The batch 12 ... 15 holds the cut at 15; its second piece raises once, the batch is retried frame by frame, and frame 15
    still gets the second scene's palette: the stream index travels with every call."""
    from dither_pie_amd import video_processor as v
    frames = clip[0]
    scenes, want = expected
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    real, calls = v.process_frames, []

    def flaky(x, ditherer, *a, **k):
        calls.append((x.shape[0], ditherer.palette))
        if len(calls) == 5:                                              # batches 0-3, 4-7, 8-11, then 12-14 | 15: the piece [15, 16)
            raise ValueError("injected: this piece fails once")
        return real(x, ditherer, *a, **k)
    monkeypatch.setattr(v, "process_frames", flaky)
    vp = v.VideoProcessor(devices=[0])
    out_path = tmp_path / "o.bin"
    assert vp._stream_through_pipes("in.mp4", str(out_path), _ditherer("bayer"), None, 64, 4, 2, vp.get_video_info("in.mp4"), overlap=overlap,
                                    scene_palettes=scenes) == 40
    assert out_path.read_bytes().split(b"\n", 1)[1] == want["bayer"].tobytes()
    assert calls[3] == (3, PALETTES[0]) and calls[4] == (1, PALETTES[1])                       # the batch, in two pieces
    assert calls[5:9] == [(1, PALETTES[0])] * 3 + [(1, PALETTES[1])]                            # retried frame by frame


def test_streaming_refusals(T, clip, tmp_path, monkeypatch):
    from dither_pie_amd.scenes import Scene
    from dither_pie_amd.video_processor import VideoProcessor
    fake_ffmpeg_tools(tmp_path, monkeypatch, clip[0][:2])
    vp = VideoProcessor(devices=[0])
    info = vp.get_video_info("in.mp4")
    started = []
    monkeypatch.setattr(VideoProcessor, "_open_decoder", lambda *a, **k: started.append(a) or (_ for _ in ()).throw(AssertionError("decoder started")))
    out = str(tmp_path / "o.bin")
    pal = PALETTES[0]
    for bad in ([], [Scene(0, 9, pal), Scene(8, 12, pal)], [Scene(0, 9, pal), Scene(9, 12, None)]):
        with pytest.raises(ValueError):
            vp._stream_through_pipes("in.mp4", out, _ditherer("bayer"), None, 64, 4, None, info, scene_palettes=bad)
        with pytest.raises(ValueError):
            vp.process_video_streaming("in.mp4", out, _ditherer("bayer"), scene_palettes=bad)
    with pytest.raises(ValueError, match="use_pipes"):
        vp.process_video_streaming("in.mp4", out, _ditherer("bayer"), use_pipes=False, scene_palettes=[Scene(0, 9, pal)])
    with pytest.raises(ValueError, match="run"):
        vp._stream_through_pipes("in.mp4", out, None, None, 64, 4, None, info, run=lambda x: x, scene_palettes=[Scene(0, 9, pal)])
    assert not started
