"""CPU tier: finished PNG chunks, their CRCs and the APNG writer without a device.  The host statements of
include/ditherpie_hip_png_file.h (through ctypes) against zlib.crc32 and the plain-Python statement of tests/png_file_ref.py;
ApngWriter(encoder="host") against that statement and against Pillow's APNG decoder; batching; refusals; the sanitizer
harness as a stand-alone program; and the agreement of the header, _lib.EXPORTS_PNG_FILE and the memory matrix of
tests/test_gpu_png_file_memory.py."""
import ctypes as C
import io
import os
import re
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import png_file_ref as fr
import png_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ditherpie_hip_png_file.h")
CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
DP_OK, DP_EINVAL, DP_EUNSUPPORTED, DP_EWORKSPACE = 0, 1, 2, 5
KS = (2, 3, 15, 16, 17, 255, 256)


@pytest.fixture(scope="module")
def be():
    from dither_pie_amd import backend
    return backend


@pytest.fixture(scope="module")
def L():
    from dither_pie_amd import _lib
    return _lib.load()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------ CRC-32
def boundary_lengths(be):
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    return sorted(set(list(range(10)) + [P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 3 * S + 1]))


def test_constants_are_those_of_the_header(be):
    text = open(HEADER).read()
    assert f"#define DP_PNG_CRC_PIECE_BYTES {be.PNG_CRC_PIECE_BYTES}\n" in text and f"#define DP_PNG_CRC_SPAN_BYTES {be.PNG_CRC_SPAN_BYTES}\n" in text
    assert be.PNG_CRC_SPAN_BYTES % be.PNG_CRC_PIECE_BYTES == 0 and be.PNG_CRC_SPAN_BYTES > be.PNG_CRC_PIECE_BYTES > 4


def test_host_crc_equals_zlib(be):
    rs = np.random.RandomState(1)
    lengths = boundary_lengths(be)
    stride = max(lengths)
    for name, data in (("noise", rs.randint(0, 256, (len(lengths), stride)).astype(np.uint8)), ("zeros", np.zeros((len(lengths), stride), np.uint8)),
                       ("ones", np.full((len(lengths), stride), 0xFF, np.uint8))):
        got = be.png_crc32_host(data, lengths)
        assert got.dtype == np.uint32 and got.shape == (len(lengths),)
        for r, n in enumerate(lengths):
            assert int(got[r]) == zlib.crc32(data[r, :n].tobytes()), (name, n)
    assert be.png_crc32_host(np.zeros((1, 0), np.uint8), [0]).tolist() == [0] == [zlib.crc32(b"")]
    assert int(be.png_crc32_host(np.frombuffer(b"123456789", np.uint8), [9])[0]) == 0xCBF43926     # the catalogue's check value
    assert be.png_crc32_host(np.zeros((0, 5), np.uint8), []).shape == (0,)
    # a size outside [0, stride] is clamped, never followed
    data = rs.randint(0, 256, (2, 40)).astype(np.uint8)
    assert be.png_crc32_host(data, [-5, 1000]).tolist() == [0, zlib.crc32(data[1].tobytes())]


def test_combine(be):
    rs = np.random.RandomState(2)
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    for la in (0, 1, 7, P, S + 3):
        for lb in (0, 1, 3, 4, P - 1, P, 1000, S, 2 * S + 1):
            a, b = rs.randint(0, 256, la).astype(np.uint8).tobytes(), rs.randint(0, 256, lb).astype(np.uint8).tobytes()
            assert be.png_crc32_combine_host(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    with pytest.raises(ValueError):
        be.png_crc32_combine_host(1, 2, -1)
    # beyond anything a test can hold in memory: against zlib's running value over zeros
    n = 1 << 24
    assert be.png_crc32_combine_host(zlib.crc32(b"abc"), zlib.crc32(bytes(n)), n) == zlib.crc32(bytes(n), zlib.crc32(b"abc"))


# ------------------------------------------------------------------------------------------------------------ assembly
def _streams(rs, lengths):
    return [rs.randint(0, 256, n).astype(np.uint8).tobytes() for n in lengths]


def _variants(rs, n):
    shared = rs.randint(0, 256, 41).astype(np.uint8).tobytes()
    each = [rs.randint(0, 256, 38).astype(np.uint8).tobytes() for _ in range(n)]
    return [(None, None), (shared, None), (each, None), (None, b"\x00\x00\x00\x00IEND\xaeB`\x82"), (shared, b"x"), (each, b"0123456789" * 6 + b"abcd")]


def _pre_arg(pre):
    return pre if pre is None or isinstance(pre, bytes) else np.frombuffer(b"".join(pre), np.uint8).reshape(len(pre), -1)


def test_assemble_host_equals_the_reference(be):
    rs = np.random.RandomState(3)
    for lengths in ([0], [5], [17, 0, 300, 1], [70000, 3, 16384, 16385]):
        n = len(lengths)
        streams = _streams(rs, lengths)
        for n_idat in sorted({0, 1, n}):
            for pre, post in _variants(rs, n):
                for seq0, step in ((0, 2), (2, 2), (4000000000, 200000000)):
                    want, woffs = fr.assemble(streams, pre, post, n_idat, seq0, step)
                    got, offs = be.png_file_assemble_host(streams, _pre_arg(pre), post, n_idat, seq0, step)
                    assert offs == woffs and got == want, (lengths, n_idat, seq0)
    assert be.png_file_assemble_host([]) == (b"", [0])
    got, offs = be.png_file_assemble_host(streams)                     # the default: every frame an IDAT chunk
    assert got == b"".join(fr.chunk(b"IDAT", s) for s in streams)
    for bad in (dict(pre=bytes(4097)), dict(post=bytes(65)), dict(n_idat=5), dict(n_idat=-1), dict(seq0=-1), dict(seq_step=1 << 32),
                dict(pre=np.zeros((3, 4), np.uint8))):
        with pytest.raises(ValueError):
            be.png_file_assemble_host(streams, **bad)


def test_helpers_and_refusals(L):
    assert L.dp_png_file_bound_bytes(1000, 38, 12) == 38 + 16 + 1000 + 12 and L.dp_png_file_bound_bytes(0, 0, 0) == 16
    assert L.dp_png_file_bound_bytes((1 << 31) - 17, 4096, 64) == (1 << 31) - 17 + 16 + 4096 + 64
    for stride, pre, post in (((1 << 31) - 16, 0, 0), (-1, 0, 0), (10, -1, 0), (10, 4097, 0), (10, 0, -1), (10, 0, 65)):
        assert L.dp_png_file_bound_bytes(stride, pre, post) == 0, (stride, pre, post)
    assert L.dp_png_file_workspace_bytes(-1, 10) == 0 and L.dp_png_file_workspace_bytes(1, (1 << 31) - 16) == 0 and L.dp_png_crc32_workspace_bytes(1, -1) == 0
    one, many = L.dp_png_file_workspace_bytes(1, 100), L.dp_png_file_workspace_bytes(7, 5 * 16384 + 1)
    assert one >= 4 and one % 16 == 0 and many >= 7 * 6 * 4 and L.dp_png_crc32_workspace_bytes(7, 5 * 16384 + 1) == many

    streams = np.arange(64, dtype=np.uint8).reshape(2, 32)
    sizes = np.array([32, 7], np.int64)
    bound = L.dp_png_file_bound_bytes(32, 3, 2)
    pre, post = np.array([1, 2, 3], np.uint8), np.array([9, 8], np.uint8)
    out, offs = np.full(2 * bound, 0xAB, np.uint8), np.full(3, -7, np.int64)
    ok = [_ptr(streams), 32, _ptr(sizes), 2, 1, 0, 2, _ptr(pre), 0, 3, _ptr(post), 2, _ptr(out), out.size, _ptr(offs)]
    names = dict(streams=0, stride=1, sizes=2, n=3, n_idat=4, pre=7, pre_stride=8, pre_bytes=9, post=10, post_bytes=11, out=12, out_bytes=13, offsets=14)

    def host(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names[key]] = v
        return L.dp_png_file_assemble_host_u8(*a)
    for kw in (dict(streams=None), dict(sizes=None), dict(out=None), dict(offsets=None), dict(pre=None), dict(post=None), dict(n=-1), dict(n_idat=-1),
               dict(n_idat=3), dict(stride=-1), dict(stride=(1 << 31) - 16), dict(pre_bytes=4097), dict(pre_bytes=-1), dict(post_bytes=65), dict(pre_stride=2),
               dict(pre_stride=-3), dict(out_bytes=2 * bound - 1)):
        assert host(**kw) == DP_EINVAL and b"dp_png_file_assemble_host_u8" in L.dp_last_error(), kw
    assert host(n=0, n_idat=0) == DP_OK
    assert (out == 0xAB).all() and (offs == -7).all()                   # nothing was touched
    assert host() == DP_OK and offs.tolist() == [0, 3 + 12 + 32 + 2, 3 + 12 + 32 + 2 + 3 + 16 + 7 + 2]
    assert host(pre=None, pre_bytes=0, post=None, post_bytes=0) == DP_OK   # NULL goes with a length of zero

    # the device entry points refuse before any HIP call: no device is needed to see it
    ws = L.dp_png_file_workspace_bytes(2, 32)
    dev = [0x1000, 32, 0x2000, 2, 1, 0, 2, 0x3000, 0, 3, 0x4000, 2, 0x5000, 2 * bound, 0x6000, 0x7000, ws, None]
    dnames = dict(names, ws=15, need=16)

    def device(**kw):
        a = list(dev)
        for key, v in kw.items():
            a[dnames[key]] = v
        rc = L.dp_png_file_assemble_u8(*a)
        assert b"dp_png_file_assemble_u8" in L.dp_last_error()
        return rc
    for kw in (dict(streams=None), dict(sizes=None), dict(out=None), dict(offsets=None), dict(ws=None), dict(pre=None), dict(post=None), dict(n=-1),
               dict(n_idat=3), dict(n_idat=-1), dict(stride=(1 << 31) - 16), dict(pre_bytes=4097), dict(post_bytes=65), dict(pre_stride=1),
               dict(out_bytes=2 * bound - 1), dict(sizes=0x2004), dict(offsets=0x6004), dict(ws=0x7008)):
        assert device(**kw) == DP_EINVAL, kw
    assert device(need=ws - 1) == DP_EWORKSPACE and device(need=0) == DP_EWORKSPACE
    assert device(n=65536, n_idat=0, out_bytes=1 << 40, need=1 << 40) == DP_EUNSUPPORTED
    assert device(n=0, n_idat=0, need=0) == DP_OK                       # n == 0: a no-op

    cws = L.dp_png_crc32_workspace_bytes(2, 32)
    cdev = [0x1000, 32, 0x2000, 2, 0x3000, 0x4000, cws, None]

    def crc(**kw):
        a = list(cdev)
        for key, v in kw.items():
            a[dict(data=0, stride=1, sizes=2, n=3, crc=4, ws=5, need=6)[key]] = v
        rc = L.dp_png_crc32_u8(*a)
        assert b"dp_png_crc32_u8" in L.dp_last_error()
        return rc
    for kw in (dict(data=None), dict(sizes=None), dict(crc=None), dict(ws=None), dict(n=-1), dict(stride=-1), dict(stride=(1 << 31) - 16),
               dict(sizes=0x2004), dict(crc=0x3002), dict(ws=0x4008)):
        assert crc(**kw) == DP_EINVAL, kw
    assert crc(need=cws - 1) == DP_EWORKSPACE and crc(n=65536, need=1 << 40) == DP_EUNSUPPORTED and crc(n=0, need=0) == DP_OK
    assert L.dp_png_crc32_host_u8(None, 32, _ptr(sizes), 2, _ptr(offs)) == DP_EINVAL


# ------------------------------------------------------------------------------------------------------------ APNG
def _clip(k, seed=0):
    rs = np.random.RandomState(100 + k + seed)
    return fr.clip(rs, 5, 13, 21, k), rs.randint(0, 256, (k, 3)).astype(np.uint8)


def _write(planes, palette, fps, cuts, **kw):
    from dither_pie_amd import apng
    f = io.BytesIO()
    with apng.ApngWriter(f, planes.shape[2], planes.shape[1], fps, encoder="host", **kw) as a:
        at = 0
        for c in cuts:
            assert a.add(planes[at:at + c], palette) == c
            at += c
    return f.getvalue()


def _reference(be, planes, palette, delta, loop, fps, seg=None, blocks="fixed"):
    _, transparent, depth = fr.apng_plan(len(palette), delta)
    todo = planes if transparent is None else fr.delta_planes(planes, transparent)
    return fr.apng_file(planes.shape[2], planes.shape[1], palette, delta, loop, fps, be.png_deflate_host(todo, depth, seg, blocks))


def _decodes(data, planes, palette, fps):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.n_frames == len(planes) and im.size == (planes.shape[2], planes.shape[1])
    num, den = fr.delay(fps)
    for f in range(len(planes)):
        im.seek(f)
        assert abs(im.info["duration"] - 1000.0 * num / den) < 1e-6, f
        assert np.array_equal(np.asarray(im.convert("RGB")), palette[planes[f]]), f


@pytest.mark.parametrize("delta", [True, False])
@pytest.mark.parametrize("k", KS)
def test_apng_host_writer(be, k, delta):
    planes, palette = _clip(k)
    assert 0.5 < (planes[1:] == planes[:-1]).mean() < 0.8
    fps = (30, Fraction(30000, 1001), 12.5)[k % 3]
    data = _write(planes, palette, fps, [5], delta=delta, loop=k % 4)
    assert data == _reference(be, planes, palette, delta, k % 4, fps)
    kinds = pr.chunks_of(data)
    keyed = delta and k <= 255
    assert [c for c, _ in kinds][:4 + keyed] == [b"IHDR", b"acTL", b"PLTE"] + [b"tRNS"] * keyed + [b"fcTL"]
    assert [c for c, _ in kinds][3 + keyed:] == [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * 4 + [b"IEND"]
    assert kinds[0][1][8] == be.png_depth(k + 1 if keyed else k) and len(kinds[2][1]) == 3 * (k + keyed)
    _decodes(data, planes, palette, fps)


def test_deltas_cost_a_depth_step_where_the_docstring_says(be):
    for k in KS + (4,):
        planes, palette = _clip(k)
        on, off = (pr.chunks_of(_write(planes, palette, 25, [5], delta=d))[0][1][8] for d in (True, False))
        assert (on > off) == (k in (2, 4, 16)), k


@pytest.mark.parametrize("delta", [True, False])
def test_batching_is_invisible(be, delta):
    for k, seg, blocks in ((15, None, "fixed"), (255, 256, "dynamic"), (256, 256, "fixed")):
        planes, palette = _clip(k, 1)
        whole = _write(planes, palette, 24, [5], delta=delta, seg_bytes=seg, blocks=blocks)
        assert whole == _write(planes, palette, 24, [1, 2, 2], delta=delta, seg_bytes=seg, blocks=blocks) == _write(planes, palette, 24, [2, 3], delta=delta, seg_bytes=seg, blocks=blocks)
        assert whole == _reference(be, planes, palette, delta, 0, 24, seg, blocks)
        _decodes(whole, planes, palette, 24)


def test_delay():
    from dither_pie_amd import apng
    assert apng.delay(30) == (1, 30) and apng.delay(25.0) == (1, 25) and apng.delay(Fraction(30000, 1001)) == (1001, 30000)
    assert apng.delay(30000 / 1001) == (1001, 30000) and apng.delay(29.97) == (100, 2997) and apng.delay(0.5) == (2, 1)
    assert apng.delay(1 / 65535) == (65535, 1) and apng.delay(65535) == (1, 65535)
    for bad in (0, -1, 1e-9, 1e9, "x", None, float("nan")):
        with pytest.raises(ValueError):
            apng.delay(bad)


def test_writer_refusals_and_the_empty_writer(tmp_path):
    import torch
    from dither_pie_amd import apng
    planes, palette = _clip(3)

    class Pipe(io.BytesIO):
        def seekable(self):
            return False
    with pytest.raises(ValueError, match="seekable"):
        apng.ApngWriter(Pipe(), 21, 13, 30, encoder="host")
    with pytest.raises(ValueError, match="seekable"):
        apng.ApngWriter(object(), 21, 13, 30, encoder="host")
    for kw in (dict(encoder="zlib"), dict(blocks="none"), dict(seg_bytes=100), dict(loop=-1), dict(fps=0)):
        args = dict(dict(fps=30, encoder="host"), **kw)
        with pytest.raises(ValueError):
            apng.ApngWriter(io.BytesIO(), 21, 13, **args)
    with pytest.raises(ValueError):
        apng.ApngWriter(io.BytesIO(), 0, 13, 30, encoder="host")
    f = io.BytesIO()
    a = apng.ApngWriter(f, 21, 13, 30, encoder="host")
    with pytest.raises(ValueError, match="do not fit"):
        a.add(planes[:, :12], palette)                                  # geometry
    with pytest.raises(ValueError, match="256 colours"):
        a.add(planes, np.zeros((257, 3), np.uint8))
    with pytest.raises(ValueError, match="one-byte"):
        a.add(planes.astype(np.int16), palette)
    assert a.add(planes[:0], palette) == 0 and f.getvalue() == b""
    assert a.add(planes[:2], palette) == 2
    other = palette.copy()
    other[1, 2] ^= 1
    before = f.getvalue()
    with pytest.raises(ValueError, match="one palette"):
        a.add(planes[2:], other)                                        # a second palette
    with pytest.raises(ValueError, match="one palette"):
        a.add(planes[2:], palette[:2])
    assert f.getvalue() == before
    a.close()
    a.close()
    with pytest.raises(ValueError, match="closed"):
        a.add(planes, palette)
    _decodes(f.getvalue(), planes[:2], palette, 30)
    with pytest.raises(ValueError, match="CUDA"):
        apng.ApngWriter(io.BytesIO(), 21, 13, 30).add(planes, palette)  # the device encoder takes CUDA planes
    with pytest.raises(ValueError, match="one-byte"):
        apng.ApngWriter(io.BytesIO(), 21, 13, 30, encoder="host").add(torch.zeros((1, 13, 21), dtype=torch.int16), palette)
    # a writer that never got a frame writes nothing
    f = io.BytesIO()
    with apng.ApngWriter(f, 21, 13, 30, encoder="host"):
        pass
    assert f.getvalue() == b""
    assert apng.write_apng(str(tmp_path / "a.png"), planes, palette, 30, encoder="host") == 5
    assert (tmp_path / "a.png").read_bytes() == _write(planes, palette, 30, [5])
    with pytest.raises(ValueError):
        apng.write_apng(str(tmp_path / "b.png"), planes[0], palette, 30, encoder="host")


def test_encode_png_host_path_is_unchanged_and_device_assembly_needs_the_device_encoder(tmp_path):
    from dither_pie_amd import png
    rs = np.random.RandomState(8)
    palette = rs.randint(0, 256, (17, 3))
    planes = rs.randint(0, 17, (3, 23, 37)).astype(np.uint8)
    files = png.encode_png(planes, palette, encoder="host")
    assert files == png.encode_png(planes, palette, encoder="host", assemble="host")
    from dither_pie_amd import backend
    assert files == [pr.container(37, 23, 8, palette, s) for s in backend.png_deflate_host(planes, 8)]
    for call in (lambda: png.encode_png(planes, palette, encoder="host", assemble="device"),
                 lambda: png.write_png(str(tmp_path / "x.png"), planes[0], palette, encoder="host", assemble="device"),
                 lambda: png.write_png_sequence(str(tmp_path / "f%d.png"), planes, palette, encoder="host", assemble="device")):
        with pytest.raises(ValueError, match="encoder='device'"):
            call()
    with pytest.raises(ValueError, match="assemble"):
        png.encode_png(planes, palette, encoder="host", assemble="gpu")
    with pytest.raises(ValueError, match="CUDA"):
        png.encode_png(planes, palette, assemble="device")
    assert list(tmp_path.iterdir()) == []


def test_process_video_apng_refuses_before_anything_starts(tmp_path, monkeypatch):
    from dither_pie_amd import video_processor as v
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    started = []
    monkeypatch.setattr(v.VideoProcessor, "_scan_decoded", lambda self, *a, **k: started.append(a))
    monkeypatch.setattr(v.VideoProcessor, "get_video_info", lambda self, *a, **k: started.append(a))
    d = ImageDitherer(4, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    out = str(tmp_path / "o.png")
    many = [(i, i, i) for i in range(256)] + [(1, 2, 3)]
    for kw in (dict(max_frames=0), dict(seg_bytes=100), dict(seg_bytes=40000), dict(blocks="none")):
        with pytest.raises(ValueError):
            v.VideoProcessor(devices=[0]).process_video_apng("in.mp4", out, d, **kw)
    with pytest.raises(ValueError, match="one device"):
        v.VideoProcessor(devices=[0, 1]).process_video_apng("in.mp4", out, d)
    with pytest.raises(ValueError, match="256"):
        v.VideoProcessor(devices=[0]).process_video_apng("in.mp4", out, ImageDitherer(257, DitherMode.BAYER, many))
    with pytest.raises(TypeError):
        v.VideoProcessor(devices=[0]).process_video_apng("in.mp4", out, d, scene_palettes=[])   # one file, one palette: no such argument
    assert started == [] and list(tmp_path.iterdir()) == []


# ------------------------------------------------------------------------------------------------------------ sanitizers
def test_host_statements_under_the_sanitizers(be, tmp_path):
    """The stand-alone harness (csrc/host_sanitize.cpp, built with -fsanitize=address,undefined) runs png_file_assemble,
    crc32_bytes and crc32_combine on buffers of exactly the sizes the header promises and prints what the library's host
    statements give."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    rs = np.random.RandomState(9)
    S = be.PNG_CRC_SPAN_BYTES
    cases = []
    for lengths, n_idat, pre_bytes, per_frame, post_bytes in (([0], 0, 0, 0, 0), ([5, 0, 64, 63], 1, 38, 1, 0), ([300, 7], 2, 41, 0, 12), ([S + 1, S - 1, 3], 0, 0, 0, 64),
                                                               ([1, 2, 3, 4, 5, 6, 7, 8, 9], 1, 4096, 1, 1)):
        n, stride = len(lengths), max(lengths)
        streams = rs.randint(0, 256, (n, stride)).astype(np.uint8)
        pre = rs.randint(0, 256, (n if per_frame else 1, pre_bytes)).astype(np.uint8)
        post = rs.randint(0, 256, post_bytes).astype(np.uint8)
        cases.append((lengths, stride, n_idat, 2 * n_idat + 1, 2, pre, per_frame, post, streams))
    with open(tmp_path / "cases.bin", "wb") as f:
        for lengths, stride, n_idat, seq0, step, pre, per_frame, post, streams in cases:
            f.write(np.array([len(lengths), stride, n_idat, seq0, step, pre.shape[1], per_frame, post.size], np.int32).tobytes())
            f.write(np.array(lengths, np.int64).tobytes() + streams.tobytes() + pre.tobytes() + post.tobytes())
    r = subprocess.run([os.path.join(CSRC, "build", "host_asan"), "pngfile", str(tmp_path / "cases.bin"), str(len(cases))], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("file ")]
    crcs = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("crc ")]
    assert len(files) == len(cases) and len(crcs) == sum(len(c[0]) for c in cases)
    at = 0
    for c, (lengths, stride, n_idat, seq0, step, pre, per_frame, post, streams) in enumerate(cases):
        runs = [streams[i, :n].tobytes() for i, n in enumerate(lengths)]
        want, _ = be.png_file_assemble_host(runs, (pre if per_frame else pre[0]) if pre.shape[1] else None, post.tobytes() or None, n_idat, seq0, step)
        assert int(files[c][1]) == c and int(files[c][2]) == len(want) and bytes.fromhex(files[c][3] if len(files[c]) > 3 else "") == want, c
        assert want == fr.assemble(runs, None if not pre.shape[1] else [p.tobytes() for p in pre] if per_frame else pre[0].tobytes(), post.tobytes(), n_idat, seq0, step)[0]
        joined = b""
        for i, run in enumerate(runs):
            joined += run
            assert (int(crcs[at][1]), int(crcs[at][2])) == (c, i) and int(crcs[at][3], 16) == zlib.crc32(run) and int(crcs[at][4], 16) == zlib.crc32(joined), (c, i)
            at += 1


# ------------------------------------------------------------------------------------------------------------ the header
def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"\b(dp_\w+)\s*\(", text)


def test_header_exports_and_memory_matrix_agree():
    import importlib
    import sys
    from dither_pie_amd import _lib
    names = _header_functions()
    assert len(names) == len(set(names)) == 8
    assert sorted(names) == sorted(_lib.EXPORTS_PNG_FILE)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF) | set(_lib.EXPORTS_PNG)
              | set(_lib.EXPORTS_PNG_DYN) | set(_lib.EXPORTS_PATTERN))
    assert not others & set(_lib.EXPORTS_PNG_FILE)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    mem = importlib.import_module("test_gpu_png_file_memory")
    device = {n for n in names if not n.endswith(("_bytes", "_host_u8", "_host"))}   # what takes device pointers
    assert device == {"dp_png_crc32_u8", "dp_png_file_assemble_u8"}
    assert set(mem.COVERAGE) | set(mem.EXCLUDED) == device and not set(mem.COVERAGE) & set(mem.EXCLUDED)
    for fn, tests in mem.COVERAGE.items():
        assert tests and all(callable(getattr(mem, t)) for t in tests), fn
    assert _lib.ABI_VERSION == 103 and _lib.load().dp_version() == 103          # additions: the revision is unchanged
    assert "#define DP_ABI_VERSION 103" in open(os.path.join(ROOT, "include", "ditherpie_hip.h")).read()
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes is not None
