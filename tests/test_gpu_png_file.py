"""GPU tier of the finished PNG chunks and the APNG output: the device CRC-32 (dp_png_crc32_u8) equals zlib.crc32 at the
boundaries of its pieces and spans, at every base alignment, with empty runs between long ones; the device assembly
(dp_png_file_assemble_u8) writes the bytes of the host statement (itself pinned to tests/png_file_ref.py by the CPU tier) on
real encoder output; encode_png(assemble="device") equals the host container with one IDAT chunk; ApngWriter on the device
equals the host writer byte for byte however the clip is cut; and process_video_apng decodes in Pillow to exactly the frames
the RGB pipeline computes."""
import io
import zlib

import numpy as np
import pytest

import png_file_ref as fr
import png_ref as pr
import scene_ref as sr
from conftest import fake_ffmpeg_tools

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


def _crc_check(T, be, data, sizes, what):
    got = be.png_crc32(T.from_numpy(data).cuda(), T.tensor(sizes, dtype=T.int64, device="cuda"))
    assert got.dtype == T.uint32 and got.shape == (len(sizes),)
    got = got.cpu().numpy().tolist()
    for r, n in enumerate(sizes):
        assert got[r] == zlib.crc32(data[r, :n].tobytes()), (what, r, n)


# ------------------------------------------------------------------------------------------------------------ CRC-32
def test_crc_at_the_piece_and_span_boundaries(T, be):
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    sizes = list(range(10)) + [P - 1, P, P + 1, 2 * P - 1, 2 * P + 1, S - 1, S, S + 1, 0, 3 * S + 1, 0, 0, 2 * S + 5, 4 * P]
    sizes += [S - 3 + k for k in range(7)] + [P - 3 + k for k in range(7)] + [0, 3 * S + 3]
    assert len(sizes) >= 40 and max(sizes) >= 3 * S + 1
    stride = max(sizes) | 1                                             # odd: run r starts at base + r (mod 4), every residue
    rs = np.random.RandomState(21)
    _crc_check(T, be, rs.randint(0, 256, (len(sizes), stride)).astype(np.uint8), sizes, "noise")
    _crc_check(T, be, np.zeros((len(sizes), stride), np.uint8), sizes, "zeros")
    _crc_check(T, be, np.full((len(sizes), stride), 0xFF, np.uint8), sizes, "ones")


@pytest.mark.parametrize("off", range(4))
def test_crc_at_every_base_alignment(T, be, off):
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    sizes = [S + 2, 1, 2, 3, 4, 5, 6, 7, P, S, 0, P + 3]
    stride = S + 3                                                      # odd
    rs = np.random.RandomState(22 + off)
    data = rs.randint(0, 256, (len(sizes), stride)).astype(np.uint8)
    buf = T.empty(data.size + 8, dtype=T.uint8, device="cuda")
    start = (off - buf.data_ptr()) % 4
    view = buf[start:start + data.size].view(data.shape)
    view.copy_(T.from_numpy(data))
    assert view.data_ptr() % 4 == off and {(view.data_ptr() + r * stride) % 4 for r in range(4)} == {0, 1, 2, 3}
    got = be.png_crc32(view, sizes).cpu().numpy().tolist()              # host integers as sizes
    assert got == [zlib.crc32(data[r, :n].tobytes()) for r, n in enumerate(sizes)]


def test_crc_clamps_sizes_and_takes_one_run(T, be):
    rs = np.random.RandomState(23)
    data = rs.randint(0, 256, (3, 77)).astype(np.uint8)
    got = be.png_crc32(T.from_numpy(data).cuda(), [-1, 77000, 77]).cpu().numpy().tolist()
    assert got == [0, zlib.crc32(data[1].tobytes()), zlib.crc32(data[2].tobytes())]
    assert be.png_crc32(T.from_numpy(data[0]).cuda(), [50]).cpu().numpy().tolist() == [zlib.crc32(data[0, :50].tobytes())]
    assert be.png_crc32(T.empty((0, 5), dtype=T.uint8, device="cuda"), []).shape == (0,)
    with pytest.raises(TypeError):
        be.png_crc32(data, [1, 2, 3])
    with pytest.raises(ValueError):
        be.png_crc32(T.from_numpy(data).cuda(), [1, 2])


# ------------------------------------------------------------------------------------------------------------ assembly
SHAPES = [((3, 17, 33), 16, "tile"), ((4, 64, 64), 4, "photo"), ((2, 37, 53), 2, "noise"), ((1, 1, 1), 2, "flat"), ((1, 600, 600), 256, "noise")]


@pytest.fixture(scope="module")
def encoded(T, be):
    """Real encoder output, computed once: {(case, seg, blocks): (payload, sizes, host streams)}"""
    made = {}
    for c, (shape, k, kind) in enumerate(SHAPES):
        planes = pr.content(kind, np.random.RandomState(30 + c), *shape, k)
        for seg in (256, 8192):
            for blocks in be.PNG_BLOCKS:
                payload, sizes = be.png_deflate(T.from_numpy(planes).cuda(), be.png_depth(k), seg, blocks)
                made[c, seg, blocks] = (payload, sizes, be.png_deflate_host(planes, be.png_depth(k), seg, blocks))
    return made


@pytest.mark.parametrize("blocks", ["fixed", "dynamic"])
@pytest.mark.parametrize("seg", [256, 8192])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_assembly_equals_the_host_statement(T, be, encoded, case, seg, blocks):
    payload, sizes, streams = encoded[case, seg, blocks]
    n = len(streams)
    assert [len(s) for s in streams] == sizes.cpu().tolist()
    rs = np.random.RandomState(40 + case)
    shared = rs.randint(0, 256, 41).astype(np.uint8)
    each = rs.randint(0, 256, (n, 38)).astype(np.uint8)
    iend = fr.chunk(b"IEND", b"")
    for n_idat in sorted({0, 1, n}):
        for pre, post in ((None, None), (shared, None), (each, iend), (T.from_numpy(each).cuda(), None), (shared.tobytes(), b"x")):
            out, offsets = be.png_file_assemble(payload, sizes, pre, post, n_idat, 2 * n_idat + 6, 2)
            assert out.dtype == T.uint8 and offsets.dtype == T.int64 and offsets.shape == (n + 1,) and out.is_cuda and offsets.is_cuda
            offsets = offsets.cpu().tolist()
            host_pre = pre.cpu().numpy() if isinstance(pre, T.Tensor) else pre
            want, woffs = be.png_file_assemble_host(streams, host_pre, post, n_idat, 2 * n_idat + 6, 2)
            assert offsets == woffs, (n_idat, type(pre))
            got = out[:offsets[-1]].cpu().numpy().tobytes()
            if got != want:
                at = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError(f"n_idat {n_idat}, prefix {type(pre).__name__}: differs from the host statement at byte {at} of {len(want)}")
    ref_pre = [e.tobytes() for e in each]
    assert want == fr.assemble(streams, shared.tobytes(), b"x", n, 2 * n + 6, 2)[0]
    assert be.png_file_assemble_host(streams, each, iend, 1, 2, 2) == fr.assemble(streams, ref_pre, iend, 1, 2, 2)


def test_assembly_wrapper_checks(T, be, encoded):
    payload, sizes, streams = encoded[0, 256, "fixed"]
    out, offsets = be.png_file_assemble(payload[:0], sizes[:0])
    assert out.numel() == 0 and offsets.cpu().tolist() == [0]
    for bad in (dict(pre=bytes(4097)), dict(post=bytes(65)), dict(n_idat=4), dict(n_idat=-1), dict(seq0=-1), dict(pre=np.zeros((2, 4), np.uint8))):
        with pytest.raises(ValueError):
            be.png_file_assemble(payload, sizes, **bad)
    with pytest.raises(TypeError):
        be.png_file_assemble(payload.cpu(), sizes)
    with pytest.raises(TypeError):
        be.png_file_assemble(payload, sizes.to(T.int32))


# ------------------------------------------------------------------------------------------------------------ PNG files
@pytest.mark.parametrize("blocks", ["fixed", "dynamic"])
def test_encode_png_assembled_on_the_device(T, be, blocks, tmp_path):
    from PIL import Image
    from dither_pie_amd import png
    rs = np.random.RandomState(50)
    for k, shape, seg in ((16, (3, 23, 37), None), (256, (2, 120, 200), 256), (2, (1, 1, 1), None)):
        palette = rs.randint(0, 256, (k, 3)).astype(np.uint8)
        planes = rs.randint(0, k, shape).astype(np.uint8)
        dev = T.from_numpy(planes).cuda()
        files = png.encode_png(dev, palette, seg, blocks=blocks, assemble="device")
        payload, sizes = be.png_deflate(dev, be.png_depth(k), seg, blocks)
        sizes = sizes.cpu().tolist()
        payload = payload.cpu().numpy()
        want = [png.container(shape[2], shape[1], be.png_depth(k), palette, payload[f, :n].tobytes(), idat_bytes=2 ** 31 - 1) for f, n in enumerate(sizes)]
        assert files == want
        assert files == png.encode_png(dev, palette, seg, blocks=blocks)  # streams below IDAT_BYTES: the host-assembled files too
        for f, data in enumerate(files):
            im = Image.open(io.BytesIO(data))
            assert im.mode == "P" and np.array_equal(np.asarray(im.convert("RGB")), palette[planes[f]])
    assert png.encode_png(dev[0], palette, assemble="device") == files[:1]
    assert png.encode_png(dev[:0], palette, assemble="device") == []
    assert png.write_png(str(tmp_path / "a.png"), dev[0], palette, assemble="device") == len(files[0]) and (tmp_path / "a.png").read_bytes() == files[0]
    paths = png.write_png_sequence(str(tmp_path / "f%02d.png"), dev, palette, start=3, assemble="device")
    assert [open(p, "rb").read() for p in paths] == png.encode_png(dev, palette, assemble="device")


def test_a_stream_longer_than_an_idat_chunk_is_one_chunk(T, be):
    from PIL import Image
    from dither_pie_amd import png
    rs = np.random.RandomState(51)
    palette = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    plane = rs.randint(0, 256, (1100, 1000)).astype(np.uint8)          # noise: the stream is stored, 1.1 MB > IDAT_BYTES
    dev = T.from_numpy(plane).cuda()
    one = png.encode_png(dev, palette, assemble="device")[0]
    cut = png.encode_png(dev, palette)[0]
    kinds_one, kinds_cut = pr.chunks_of(one), pr.chunks_of(cut)
    assert [k for k, _ in kinds_one] == [b"IHDR", b"PLTE", b"IDAT", b"IEND"] and [k for k, _ in kinds_cut] == [b"IHDR", b"PLTE", b"IDAT", b"IDAT", b"IEND"]
    assert kinds_one[2][1] == kinds_cut[2][1] + kinds_cut[3][1] and len(kinds_one[2][1]) > png.IDAT_BYTES
    assert one == png.container(1000, 1100, 8, palette, kinds_one[2][1], idat_bytes=2 ** 31 - 1)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(one)).convert("RGB")), palette[plane])


def test_assemble_passes_through_the_ditherer_and_process_frames_png(T):
    from PIL import Image
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.video_processor import process_frames_png
    rs = np.random.RandomState(52)
    d = ImageDitherer(4, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 30, 200)], dither_params={"size": "4x4"})
    frames = rs.randint(0, 256, (3, 24, 40, 3)).astype(np.uint8)
    x = T.from_numpy(frames).cuda()
    assert process_frames_png(x, d, assemble="device") == process_frames_png(x, d)
    image = Image.fromarray(frames[0])
    assert d.apply_dithering_png(image, assemble="device") == d.apply_dithering_png(image)


# ------------------------------------------------------------------------------------------------------------ APNG
def _write(planes, palette, cuts, encoder, **kw):
    from dither_pie_amd import apng
    f = io.BytesIO()
    with apng.ApngWriter(f, planes.shape[2], planes.shape[1], 30, encoder=encoder, **kw) as a:
        at = 0
        for c in cuts:
            a.add(planes[at:at + c], palette)
            at += c
    return f.getvalue()


@pytest.mark.parametrize("delta", [True, False])
@pytest.mark.parametrize("k", [3, 16, 255, 256])
def test_apng_device_writer_equals_the_host_writer(T, k, delta):
    from PIL import Image
    rs = np.random.RandomState(60 + k)
    planes = fr.clip(rs, 6, 13, 21, k)
    palette = rs.randint(0, 256, (k, 3)).astype(np.uint8)
    dev = T.from_numpy(planes).cuda()
    blocks = "dynamic" if k == 16 else "fixed"
    want = _write(planes, palette, [6], "host", delta=delta, blocks=blocks, seg_bytes=256)
    assert _write(dev, palette, [6], "device", delta=delta, blocks=blocks, seg_bytes=256) == want
    assert _write(dev, palette, [1, 2, 3], "device", delta=delta, blocks=blocks, seg_bytes=256) == want
    im = Image.open(io.BytesIO(want))
    assert im.n_frames == 6
    for f in range(6):
        im.seek(f)
        assert np.array_equal(np.asarray(im.convert("RGB")), palette[planes[f]]), f


def test_write_apng_on_the_device(T, tmp_path):
    from dither_pie_amd import apng
    rs = np.random.RandomState(61)
    planes = fr.clip(rs, 4, 40, 64, 15)
    palette = rs.randint(0, 256, (15, 3)).astype(np.uint8)
    assert apng.write_apng(str(tmp_path / "a.png"), T.from_numpy(planes).cuda(), palette, 30000 / 1001, loop=2) == 4
    assert apng.write_apng(str(tmp_path / "h.png"), planes, palette, 30000 / 1001, loop=2, encoder="host") == 4
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "h.png").read_bytes()
    with pytest.raises(ValueError, match="CUDA"):
        apng.write_apng(str(tmp_path / "b.png"), T.from_numpy(planes).cuda(), palette, 30, encoder="host")


@pytest.mark.parametrize("batch", [4, 15])                              # 40 frames: ten batches, or two and a short third
def test_process_video_apng(T, tmp_path, monkeypatch, batch):
    from PIL import Image
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.video_processor import VideoProcessor, process_frames
    frames = sr.three_scene_clip()[0]
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", batch * sr.H * sr.W * 3)
    d = ImageDitherer(5, DitherMode.BAYER, [(10, 20, 30), (70, 200, 40), (40, 90, 200), (75, 230, 250), (250, 250, 250)], dither_params={"size": "4x4"})
    want = process_frames(T.from_numpy(frames).cuda(), d, None, 64, 2).cpu().numpy()
    vp = VideoProcessor(devices=[0])
    files = {}
    for delta in (True, False):
        path = tmp_path / f"o{int(delta)}.png"
        assert vp.process_video_apng("in.mp4", str(path), d, None, 64, 2, delta=delta, seg_bytes=1024) == len(frames)
        assert vp.last_apng_stats["mode"] == "apng" and vp.last_apng_stats["bytes"] == path.stat().st_size and vp.last_scan_stats["batch_frames"] == batch
        files[delta] = path.read_bytes()
        im = Image.open(io.BytesIO(files[delta]))
        assert im.n_frames == len(frames) and im.size == (2 * sr.W, 2 * sr.H)
        for i in range(len(frames)):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert("RGB")), want[i]), (batch, delta, i)
    assert [b"tRNS" in [k for k, _ in pr.chunks_of(files[delta])] for delta in (True, False)] == [True, False]
    short = tmp_path / "short.png"
    assert vp.process_video_apng("in.mp4", str(short), d, final_resize_multiplier=2, max_frames=9, blocks="dynamic") == 9
    im = Image.open(io.BytesIO(short.read_bytes()))
    assert im.n_frames == 9
    for i in range(9):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), want[i]), i


def test_process_video_apng_raises_on_a_failed_batch(T, tmp_path, monkeypatch):
    from dither_pie_amd import video_processor as v
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    frames = sr.three_scene_clip()[0]
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(v.VideoProcessor, "PIPE_SLOT_BYTES", 4 * sr.H * sr.W * 3)
    d = ImageDitherer(2, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    real, calls = v.process_frames_indexed, []

    def flaky(x, *a, **k):
        calls.append(x.shape[0])
        if len(calls) == 3:
            raise ValueError("injected: this batch fails")
        return real(x, *a, **k)
    monkeypatch.setattr(v, "process_frames_indexed", flaky)
    with pytest.raises(ValueError, match="injected"):
        v.VideoProcessor(devices=[0]).process_video_apng("in.mp4", str(tmp_path / "o.png"), d)
    assert calls == [4, 4, 4]                                            # no frame-by-frame retry, nothing after the failure
