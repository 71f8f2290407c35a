"""GPU tier: the PNG-8 output on the device.  backend.png_deflate writes the bytes of the host statement
(backend.png_deflate_host, itself judged by zlib, the walker and Pillow in tests/test_png_cpu.py) on the named cases and on
random ones, alone and in batches with different content per frame; batching is invisible; files written by encode_png,
apply_dithering_png, process_frames_png and process_video_pngs decode in Pillow to what the RGB routes give.
Runs on the product library.  No test here is meant to fault."""
import io
import zlib

import numpy as np
import pytest

import png_ref as pr
import scene_ref as sr
from conftest import fake_ffmpeg_tools

pytestmark = pytest.mark.gpu

N_RANDOM = 40


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


def _at_offset(T, a, off):
    """The array on the device at a base address = off (mod 4): a slice of a byte buffer."""
    a = np.ascontiguousarray(a, np.uint8)
    buf = T.empty(a.size + 8, dtype=T.uint8, device="cuda")
    start = (off - buf.data_ptr()) % 4
    view = buf[start:start + a.size].view(a.shape)
    view.copy_(T.from_numpy(a))
    assert view.data_ptr() % 4 == off
    return view


def _encode(T, be, planes, depth, seg, off=1):
    payload, sizes = be.png_deflate(_at_offset(T, planes, off), depth, seg)
    assert payload.dtype == T.uint8 and sizes.dtype == T.int64
    assert payload.shape == (len(planes), be.png_deflate_stride(planes.shape[1], planes.shape[2], depth, seg))
    sizes = sizes.cpu().tolist()
    payload = payload.cpu().numpy()
    return [payload[f, :n].tobytes() for f, n in enumerate(sizes)]


def _same(got, want, what):
    assert [len(b) for b in got] == [len(b) for b in want], what
    for f, (a, b) in enumerate(zip(got, want)):
        if a != b:
            at = next(i for i in range(len(a)) if a[i] != b[i])
            raise AssertionError(f"{what}: frame {f} differs from the host statement at byte {at} of {len(a)}")


def _three(planes, rs):
    """Three frames of different content around a case's first plane."""
    h, w = planes.shape[1:]
    k = int(planes.max()) + 1
    return np.concatenate([planes[:1], pr.content("photo", rs, 1, h, w, max(k, 2)), planes[:1][:, ::-1, ::-1]])


# ---------------------------------------------------------------------------------------------------- encoder bytes
def test_encoder_equals_the_host_statement_on_the_named_cases(T, be):
    rs = np.random.RandomState(21)
    for name, planes, depth, seg in pr.named_cases():
        _same(_encode(T, be, planes, depth, seg), be.png_deflate_host(planes, depth, seg), name)
        three = _three(planes, rs)
        got = _encode(T, be, three, depth, seg, off=3)
        _same(got, be.png_deflate_host(three, depth, seg), name + " x3")
        assert zlib.decompress(got[1]) == pr.filtered(three[1], depth), name


def test_encoder_on_random_cases(T, be):
    rs = np.random.RandomState(22)
    for i, (name, planes, depth, seg) in enumerate(pr.random_cases(N_RANDOM, seed=13)):
        _same(_encode(T, be, planes[:1], depth, seg, off=i % 4), be.png_deflate_host(planes[:1], depth, seg), name)
        three = _three(planes, rs)
        _same(_encode(T, be, three, depth, seg, off=(i + 1) % 4), be.png_deflate_host(three, depth, seg), name + " x3")


@pytest.mark.parametrize("n, h, w, depth, why", [
    (10, 300, 300, 8, "353 segments a frame: the layout kernel carries offsets and Adler sums over six steps of 64; 3530 in the call: the "
                      "segment kernel's waves take a second segment on the LDS they used"),
    (1, 520, 520, 8, "1059 segments in one frame: the pack kernel strides over them"),
    (3, 700, 1001, 1, "depth 1 over many rows: 349 segments a frame with 2.03 rows each")])
def test_many_segments_equal_the_host_statement(T, be, n, h, w, depth, why):
    """The paths only the device has -- more than 64 segments a frame, more segments than resident waves, more segments a
    frame than pack workgroups -- at seg_bytes 256, where a small frame has that many."""
    rs = np.random.RandomState(25)
    k = 1 << min(depth, 4)
    planes = np.concatenate([pr.content(pr.KINDS[f % 4], rs, 1, h, w, k if f % 2 else 1 << depth) for f in range(n)])
    F = pr.filtered_size(h, w, depth)
    assert pr.n_segments(F, 256) > (1024 if n == 1 else 64) and (n != 10 or n * pr.n_segments(F, 256) > 3072), why
    got = _encode(T, be, planes, depth, 256, off=1)
    _same(got, be.png_deflate_host(planes, depth, 256), why)
    for f in (0, n - 1):
        assert zlib.decompress(got[f]) == pr.filtered(planes[f], depth)


def test_a_batch_is_its_frames_one_by_one(T, be):
    rs = np.random.RandomState(23)
    planes = np.concatenate([pr.content(kind, rs, 2, 70, 101, 16) for kind in pr.KINDS])        # 8 frames, 4 kinds
    for depth, seg in ((4, 512), (8, 8192)):
        together = _encode(T, be, planes, depth, seg)
        alone = [_encode(T, be, planes[f:f + 1], depth, seg)[0] for f in range(len(planes))]
        assert together == alone
        assert together[:3] == _encode(T, be, planes[:3], depth, seg, off=2)


def test_out_of_range_indices_are_masked(T, be):
    rs = np.random.RandomState(24)
    p = rs.randint(0, 256, (2, 19, 45)).astype(np.uint8)
    for depth in pr.DEPTHS:
        got = _encode(T, be, p, depth, 256)
        assert got == _encode(T, be, p & ((1 << depth) - 1), depth, 256) == be.png_deflate_host(p, depth, 256)


def test_argument_checks_of_the_wrapper(T, be):
    p = T.zeros((2, 4, 4), dtype=T.uint8, device="cuda")
    with pytest.raises(TypeError):
        be.png_deflate(p.cpu(), 8)
    with pytest.raises(TypeError):
        be.png_deflate(p.to(T.int16), 8)
    for depth, seg in ((3, None), (8, 255), (8, 32769)):
        with pytest.raises(ValueError):
            be.png_deflate(p, depth, seg)
    payload, sizes = be.png_deflate(p[:0], 8)
    assert payload.shape[0] == 0 and sizes.numel() == 0
    one = be.png_deflate(p[0], 8)[1]
    assert one.shape == (1,)


# ---------------------------------------------------------------------------------------------------- through the layers
def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "P"
    return im, np.asarray(im.convert("RGB")).copy()


@pytest.mark.parametrize("k", [16, 256])
def test_encode_png_decodes_to_the_palette_of_the_planes(T, tmp_path, k):
    from dither_pie_amd import png
    rs = np.random.RandomState(31)
    palette = rs.randint(0, 256, (k, 3)).astype(np.uint8)
    planes = np.concatenate([pr.content("photo", rs, 2, 96, 130, k), pr.content("noise", rs, 1, 96, 130, k)])
    dev = T.from_numpy(planes).cuda()
    files = png.encode_png(dev, palette)
    assert len(files) == 3 and files == png.encode_png(planes, palette, encoder="host")
    for f, data in enumerate(files):
        im, got = _decode(data)
        assert im.size == (130, 96) and np.array_equal(got, palette[planes[f]])
        assert pr.chunks_of(data)[0][1][8] == pr.depth_of(k) and len(pr.chunks_of(data)[1][1]) == 3 * k
    assert png.write_png(str(tmp_path / "s.png"), dev[1], palette) == len(files[1]) and (tmp_path / "s.png").read_bytes() == files[1]
    paths = png.write_png_sequence(str(tmp_path / "frame_%05d.png"), dev, palette)
    assert [p[-15:] for p in paths] == ["frame_00001.png", "frame_00002.png", "frame_00003.png"]
    assert [open(p, "rb").read() for p in paths] == files
    with pytest.raises(ValueError, match="one-byte"):
        png.encode_png(dev.to(T.int16), palette)
    with pytest.raises(ValueError, match="host arrays"):
        png.encode_png(dev, palette, encoder="host")


@pytest.mark.parametrize("mode", ["bayer", "fs"])
@pytest.mark.parametrize("use_gamma", [False, True])
def test_apply_dithering_png_decodes_to_apply_dithering(T, mode, use_gamma):
    from PIL import Image
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    rs = np.random.RandomState(32)
    y, x = np.mgrid[0:75, 0:101]
    img = Image.fromarray(np.stack([(x * 3) % 256, (y * 4) % 256, (x + y) % 256], axis=-1).astype(np.uint8), "RGB")
    pal = [tuple(int(v) for v in c) for c in rs.randint(0, 256, (13, 3))]
    d = (ImageDitherer(13, DitherMode.BAYER, pal, use_gamma=use_gamma, dither_params={"size": "4x4"}) if mode == "bayer" else
         ImageDitherer(13, DitherMode.ERROR_DIFFUSION, pal, use_gamma=use_gamma, dither_params={"variant": "floyd_steinberg"}))
    want = np.asarray(d.apply_dithering(img))
    data = d.apply_dithering_png(img)
    im, got = _decode(data)
    assert isinstance(data, bytes) and im.size == (101, 75) and np.array_equal(got, want)
    assert pr.chunks_of(data)[0][1][8] == 4                             # 13 colours: depth 4
    with pytest.raises(ValueError, match="256"):
        ImageDitherer(300, DitherMode.BAYER, [(i % 256, i // 256, 0) for i in range(300)]).apply_dithering_png(img)


def test_process_frames_png_decodes_to_process_frames(T):
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.video_processor import process_frames, process_frames_png
    rs = np.random.RandomState(33)
    frames = T.from_numpy(rs.randint(0, 256, (3, 90, 120, 3)).astype(np.uint8)).cuda()
    d = ImageDitherer(5, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 200, 30), (30, 30, 200)], dither_params={"size": "4x4"})
    want = process_frames(frames, d, "regular", 48, 3).cpu().numpy()
    files = process_frames_png(frames, d, "regular", 48, 3)
    assert len(files) == 3
    for i, data in enumerate(files):
        assert np.array_equal(_decode(data)[1], want[i])


PALETTES = [[(10, 20, 30), (70, 200, 40), (40, 90, 200), (75, 230, 250)], [(100, 0, 0), (150, 250, 250), (120, 120, 120)],
            [(180, 0, 0), (250, 250, 250), (200, 100, 50), (255, 0, 255), (181, 250, 250)]]


@pytest.fixture(scope="module")
def scene_clip(T):
    """The synthetic three-scene clip of the scene tests and process_frames scene by scene on it (Bayer 4x4, final x2)."""
    import copy
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.scenes import Scene
    from dither_pie_amd.video_processor import process_frames
    frames = sr.three_scene_clip()[0]
    scenes = [Scene(0, 15, PALETTES[0]), Scene(15, 20, PALETTES[1]), Scene(20, 36, PALETTES[2])]   # 36 ... 39 lie past the last end
    base = ImageDitherer(16, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    out = []
    for k, s in enumerate(scenes):
        d = copy.copy(base)
        d.palette = list(s.palette)
        hi = len(frames) if k == len(scenes) - 1 else s.end
        out.append(process_frames(T.from_numpy(frames[s.start:hi]).cuda(), d, None, 64, 2).cpu().numpy())
    return frames, scenes, base, np.concatenate(out)


def test_process_video_pngs_on_the_three_scene_clip(T, scene_clip, tmp_path, monkeypatch):
    from dither_pie_amd.video_processor import VideoProcessor, process_frames
    frames, scenes, base, want = scene_clip
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", 4 * sr.H * sr.W * 3)     # the cut at 15 inside a batch, at 20 on an edge
    vp = VideoProcessor(devices=[0])
    out = tmp_path / "seq"
    out.mkdir()
    assert vp.process_video_pngs("in.mp4", str(out / "frame_%05d.png"), base, None, 64, 2, scene_palettes=scenes, seg_bytes=1000) == 40
    assert base.palette == [(0, 0, 0), (255, 255, 255)] and vp.last_png_stats["mode"] == "png"
    names = sorted(p.name for p in out.iterdir())
    assert names == [f"frame_{i:05d}.png" for i in range(1, 41)]
    depths = []
    for i in range(40):
        data = (out / names[i]).read_bytes()
        im, got = _decode(data)
        assert im.size == (2 * sr.W, 2 * sr.H) and np.array_equal(got, want[i]), i
        depths.append((pr.chunks_of(data)[0][1][8], len(pr.chunks_of(data)[1][1]) // 3))
    assert depths[0] == (2, 4) and depths[15] == (2, 3) and depths[20] == (4, 5)               # the palette switches with the scene
    assert vp.last_png_stats["bytes"] == sum((out / n).stat().st_size for n in names)
    one = tmp_path / "one"
    one.mkdir()
    assert vp.process_video_pngs("in.mp4", str(one / "f%03d.png"), base, final_resize_multiplier=2, max_frames=9, start=0) == 9
    alone = process_frames(T.from_numpy(frames[:9]).cuda(), base, None, 64, 2).cpu().numpy()
    assert sorted(p.name for p in one.iterdir()) == [f"f{i:03d}.png" for i in range(9)]
    assert all(np.array_equal(_decode((one / f"f{i:03d}.png").read_bytes())[1], alone[i]) for i in range(9))


def test_process_video_pngs_raises_on_a_failed_batch(T, scene_clip, tmp_path, monkeypatch):
    from dither_pie_amd import video_processor as v
    frames, scenes, base, _ = scene_clip
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(v.VideoProcessor, "PIPE_SLOT_BYTES", 4 * sr.H * sr.W * 3)
    real, calls = v.process_frames_indexed, []

    def flaky(x, *a, **k):
        calls.append(x.shape[0])
        if len(calls) == 3:
            raise ValueError("injected: this batch fails")
        return real(x, *a, **k)
    monkeypatch.setattr(v, "process_frames_indexed", flaky)
    out = tmp_path / "seq"
    out.mkdir()
    with pytest.raises(ValueError, match="injected"):
        v.VideoProcessor(devices=[0]).process_video_pngs("in.mp4", str(out / "f_%05d.png"), base)
    assert calls == [4, 4, 4] and len(list(out.iterdir())) == 8          # no frame-by-frame retry, nothing after the failure
