"""GPU tier of the animated GIF output: the device encoder (dp_gif_lzw_encode_u8) writes the bytes of the host statement
(dp_gif_lzw_host_u8, itself pinned to tests/gif_ref.py by the CPU tier) on the named cases, the sub-block edges and 60 seeded
random cases, in batches of 1, 3 and 17 frames, at odd addresses and over pre-filled buffers; the delta kernel equals numpy and
DeltaStream makes batching invisible; files written by write_gif, GifWriter.add and process_video_gif decode in Pillow to
exactly the frames the RGB pipeline computes."""
import io

import numpy as np
import pytest

import gif_ref as gr
import scene_ref as sr
from conftest import fake_ffmpeg_tools

pytestmark = pytest.mark.gpu

N_RANDOM = 60


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


def _encode(T, be, planes, mcs, chunk, off=1):
    payload, sizes = be.gif_lzw(_at_offset(T, planes, off), mcs, chunk)
    assert payload.dtype == T.uint8 and sizes.dtype == T.int64 and payload.shape == (len(planes), be.gif_lzw_stride(planes.shape[1], planes.shape[2], chunk))
    sizes = sizes.cpu().tolist()
    payload = payload.cpu().numpy()
    return [payload[f, :n].tobytes() for f, n in enumerate(sizes)]


def _same(got, want, what):
    assert [len(b) for b in got] == [len(b) for b in want], what
    for f, (a, b) in enumerate(zip(got, want)):
        if a != b:
            at = next(i for i in range(len(a)) if a[i] != b[i])
            raise AssertionError(f"{what}: frame {f} differs from the host statement at byte {at} of {len(a)}")


# ---------------------------------------------------------------------------------------------------- encoder bytes
def test_encoder_equals_the_host_statement_on_the_named_cases(T, be):
    for name, planes, mcs, chunk in gr.named_cases():
        for off in (0, 1, 3):
            _same(_encode(T, be, planes, mcs, chunk, off), be.gif_lzw_host(planes, mcs, chunk), (name, off))


def test_encoder_at_the_sub_block_edges(T, be):
    edges = gr.subblock_edge_cases()
    assert sorted(edges) == [254, 255, 256, 509, 510, 511]
    for d, (plane, chunk) in edges.items():
        got = _encode(T, be, plane, 8, chunk, d % 4)
        _same(got, be.gif_lzw_host(plane, 8, chunk), d)
        assert len(got[0]) == 1 + d + (d + 254) // 255 + 1 and got[0][-1] == 0 and got[0][0] == 8


def test_encoder_on_random_cases(T, be):
    for seed in range(N_RANDOM):
        planes, mcs, chunk = gr.random_case(seed)
        _same(_encode(T, be, planes, mcs, chunk, seed % 4), be.gif_lzw_host(planes, mcs, chunk), seed)


@pytest.mark.parametrize("n", [1, 3, 17])
def test_batches_of_frames_with_different_contents(T, be, n):
    rs = np.random.RandomState(100 + n)
    h, w = 37, 53
    kinds = ("noise", "tile", "flat")
    planes = np.concatenate([gr.content(kinds[i % 3], rs, 1, h, w, 16) for i in range(n)])   # sizes differ within the batch
    for chunk in (64, 700, h * w):
        got = _encode(T, be, planes, 4, chunk, 1)
        _same(got, be.gif_lzw_host(planes, 4, chunk), (n, chunk))
        if n > 1:
            assert len(set(len(b) for b in got)) > 1


def test_out_of_range_indices_are_reduced(T, be):
    planes = np.random.RandomState(5).randint(0, 256, (2, 20, 23)).astype(np.uint8)
    _same(_encode(T, be, planes, 3, 50), be.gif_lzw_host(planes & 7, 3, 50), "indices past the table")


def test_a_prefilled_output_comes_out_the_same(T, be):
    from dither_pie_amd import _lib
    L = _lib.load()
    rs = np.random.RandomState(9)
    planes = gr.content("tile", rs, 3, 33, 47, 16)
    chunk, mcs = 200, 4
    want = be.gif_lzw_host(planes, mcs, chunk)
    x = _at_offset(T, planes, 1)
    stride = be.gif_lzw_stride(33, 47, chunk)
    need = L.dp_gif_lzw_workspace_bytes(3, 33, 47, chunk)
    fills = {"zeros": lambda: T.zeros((3, stride), dtype=T.uint8, device="cuda"),
             "ones": lambda: T.full((3, stride), 255, dtype=T.uint8, device="cuda"),
             "noise": lambda: T.randint(0, 256, (3, stride), device="cuda").to(T.uint8)}
    for fill, make in fills.items():
        out = make()
        ws = T.randint(0, 256, (need + 16,), device="cuda").to(T.uint8)
        ws = ws[(-ws.data_ptr()) % 16:][:need]
        sizes = T.full((3,), -7, dtype=T.int64, device="cuda")
        rc = L.dp_gif_lzw_encode_u8(x.data_ptr(), 3, 33, 47, mcs, chunk, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), need, be._stream())
        T.cuda.synchronize()
        assert rc == 0, L.dp_last_error()
        got = [out[f, :int(sizes[f])].cpu().numpy().tobytes() for f in range(3)]
        _same(got, want, fill)


def test_argument_checks_of_the_wrapper(T, be):
    ok = T.zeros((2, 4, 5), dtype=T.uint8, device="cuda")
    for planes, mcs, chunk in ((ok.cpu(), 4, None), (ok.to(T.int16), 4, None), (ok[0, 0], 4, None), (ok, 1, None), (ok, 9, None), (ok, 4, 0)):
        with pytest.raises((TypeError, ValueError)):
            be.gif_lzw(planes, mcs, chunk)
    payload, sizes = be.gif_lzw(ok[:0], 4)
    assert payload.shape[0] == 0 and sizes.shape == (0,)


# ---------------------------------------------------------------------------------------------------- delta
@pytest.mark.parametrize("h, w", [(1, 1), (3, 5), (37, 53), (64, 64)])
def test_delta_equals_numpy(T, be, h, w):
    rs = np.random.RandomState(h * 100 + w)
    for n in (1, 4):
        planes = rs.randint(0, 5, (n, h, w)).astype(np.uint8)
        if n > 2:
            planes[2] = planes[1]
        before = rs.randint(0, 5, (h, w)).astype(np.uint8)
        for off in (0, 1, 2, 3):
            for has_prev in (0, 1):
                prev = _at_offset(T, before, (off + 1) % 4) if has_prev else None
                out, changed = be.index_delta(_at_offset(T, planes, off), prev, 77)
                want, counts = gr.index_delta(planes, 77, before if has_prev else None)
                assert np.array_equal(out.cpu().numpy(), want) and changed.cpu().tolist() == counts.tolist(), (n, off, has_prev)
                if has_prev:
                    assert np.array_equal(prev.cpu().numpy(), planes[-1])      # the carried plane moved on
    x = _at_offset(T, planes, 0)
    with pytest.raises(Exception, match="in-place"):
        be.index_delta(x, None, 3, out=x)
    for bad in (256, -1):
        with pytest.raises(ValueError):
            be.index_delta(x, None, bad)


def test_delta_stream_makes_batching_invisible(T, be):
    rs = np.random.RandomState(31)
    planes = rs.randint(0, 4, (40, 17, 23)).astype(np.uint8)
    planes[11] = planes[10]
    want, counts = gr.index_delta(planes, 9)
    assert counts[11] == 0 and counts[0] == 17 * 23
    x = T.from_numpy(planes).cuda()
    for sizes in ((40,), (7, 33), (1,) * 40):
        s = be.DeltaStream()
        outs, cnts, at = [], [], 0
        for n in sizes:
            o, c = s.add(x[at:at + n], 9)
            outs.append(o.cpu().numpy())
            cnts += c.cpu().tolist()
            at += n
        assert np.array_equal(np.concatenate(outs), want) and cnts == counts.tolist(), sizes
    o, c = s.reset().add(x[5:7], 9)                                     # reset() forgets the carried plane
    assert np.array_equal(o.cpu().numpy(), gr.index_delta(planes[5:7], 9)[0]) and c.cpu().tolist() == [17 * 23, int(counts[6])]
    o, c = s.add(x[7:8], 9)
    assert np.array_equal(o.cpu().numpy(), want[7:8])
    with pytest.raises(ValueError, match="reset"):
        s.add(x[:1, :5], 9)
    o, c = s.add(x[:0], 9)
    assert o.shape[0] == 0 and c.shape == (0,)


# ---------------------------------------------------------------------------------------------------- end to end
def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    frames = []
    for i in range(im.n_frames):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return im, frames


def _clip_24(seed=3):
    """24 frames of 48 x 64: a smooth moving gradient, so that ordered and diffused dithers both have something to do."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:48, 0:64]
    frames = []
    for t in range(24):
        f = np.stack([(x * 4 + 3 * t) % 256, (y * 5 + 2 * t) % 256, ((x + y) * 2 + 5 * t) % 256], axis=-1).astype(np.uint8)
        f[10:20, 5 + t:15 + t] = rs.randint(0, 256, 3)
        frames.append(f)
    frames[13] = frames[12].copy()                                      # a repeated frame
    return np.stack(frames)


@pytest.mark.parametrize("kind", ["bayer16", "fs256"])
def test_write_gif_decodes_to_the_dithered_frames(T, tmp_path, kind):
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.gif import write_gif
    rs = np.random.RandomState(41)
    k = 16 if kind == "bayer16" else 256
    pal = [tuple(int(v) for v in c) for c in rs.randint(0, 256, (k, 3))]
    d = (ImageDitherer(k, DitherMode.BAYER, pal, dither_params={"size": "4x4"}) if kind == "bayer16" else
         ImageDitherer(k, DitherMode.ERROR_DIFFUSION, pal, dither_params={"variant": "floyd_steinberg"}))
    x = T.from_numpy(_clip_24()).cuda()
    want = d.apply_dithering_frames(x).cpu().numpy()
    planes, colours = d.apply_dithering_frames_indexed(x)
    sizes = {}
    for delta in (True, False):
        path = tmp_path / f"{kind}{int(delta)}.gif"
        assert write_gif(str(path), planes, colours, 25, delta=delta) == 24
        data = path.read_bytes()
        im, got = _decode(data)
        assert im.n_frames == 24 and im.info["duration"] == 40 and im.info["loop"] == 0
        for i in range(24):
            assert np.array_equal(got[i], want[i]), (kind, delta, i)
        sizes[delta] = len(data)
        host = tmp_path / "host.gif"
        write_gif(str(host), planes.cpu().numpy(), colours, 25, delta=delta, encoder="host")
        assert host.read_bytes() == data                                # the device's file is the host statement's file
    if k <= 255:
        assert sizes[True] < sizes[False]


@pytest.mark.parametrize("which", ["halftone", "wavelet"])
def test_halftone_and_wavelet_planes_through_the_writer(T, which):
    from dither_pie_amd import dithering_lib as dl
    from dither_pie_amd.gif import GifWriter
    rs = np.random.RandomState(43)
    frames = T.from_numpy(_clip_24()[:3, :20, :26].copy()).cuda()
    pal = [tuple(int(v) for v in c) for c in rs.randint(0, 256, (12, 3))]
    s = dl.HalftoneDitherStrategy(cell_size=5, angle=30.0) if which == "halftone" else dl.WaveletDitherStrategy("db2", 6, 9)
    want = s.dither_frames(frames, pal, False).cpu().numpy()
    planes, colours = s.dither_frames_indexed(frames, pal, False)
    buf = io.BytesIO()
    with GifWriter(buf, 26, 20, 10) as g:
        assert g.add(planes[:1], colours) == 1 and g.add(planes[1:], colours) == 2
    im, got = _decode(buf.getvalue())
    assert im.n_frames == 3 and all(np.array_equal(got[i], want[i]) for i in range(3))


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


@pytest.mark.parametrize("batch", [4, 15])                              # 4: the cut at 15 inside a batch, at 20 on an edge; 15: the first cut on an edge
def test_process_video_gif_on_the_three_scene_clip(T, scene_clip, tmp_path, monkeypatch, batch):
    from dither_pie_amd.video_processor import VideoProcessor
    frames, scenes, base, want = scene_clip
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", batch * sr.H * sr.W * 3)
    vp = VideoProcessor(devices=[0])
    for delta in (True, False):
        path = tmp_path / f"o{int(delta)}.gif"
        assert vp.process_video_gif("in.mp4", str(path), base, None, 64, 2, scene_palettes=scenes, delta=delta, chunk_px=1000) == 40
        assert vp.last_scan_stats["batch_frames"] == batch and base.palette == [(0, 0, 0), (255, 255, 255)]
        im, got = _decode(path.read_bytes())
        assert im.n_frames == 40 and im.size == (2 * sr.W, 2 * sr.H) and im.info["duration"] == 40
        for i in range(40):
            assert np.array_equal(got[i], want[i]), (batch, delta, i)
    one = tmp_path / "one.gif"                                           # without scenes: the ditherer's own palette, max_frames
    assert vp.process_video_gif("in.mp4", str(one), base, final_resize_multiplier=2, max_frames=9) == 9
    from dither_pie_amd.video_processor import process_frames
    alone = process_frames(T.from_numpy(frames[:9]).cuda(), base, None, 64, 2).cpu().numpy()
    im, got = _decode(one.read_bytes())
    assert im.n_frames == 9 and all(np.array_equal(got[i], alone[i]) for i in range(9))


def test_process_video_gif_raises_on_a_failed_batch(T, scene_clip, tmp_path, monkeypatch):
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
    with pytest.raises(ValueError, match="injected"):
        v.VideoProcessor(devices=[0]).process_video_gif("in.mp4", str(tmp_path / "o.gif"), base)
    assert calls == [4, 4, 4]                                            # no frame-by-frame retry, nothing after the failure
