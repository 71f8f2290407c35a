"""CPU tier: the PNG-8 output without a device.  The host statement of the stream (dp_png_deflate_host_u8, through ctypes)
against zlib.decompress, the walker of tests/png_ref.py and Pillow; the framing, independence and block-type rules of
include/ditherpie_hip_png.h; the size conditions; refusals, bounds and the workspace helper; the container of
dither_pie_amd/png.py; the host statement under the sanitizers as a stand-alone program; and the agreement of the header,
_lib.EXPORTS_PNG and the memory matrix of tests/test_gpu_png_memory.py.

Dynamic-Huffman blocks are not written by this revision of the encoder (stored and fixed only): the sizes are therefore
measured against zlib with Z_FIXED at level 1, and the named cases that exist for the code construction (Fibonacci counts,
one distance code, one distinct literal, the 20-byte segment, the code-length runs of 3 / 6 / 7 / 10 / 11 / 138 / 139 zeros and
repeats) are kept as stream cases; the walker's limits on code lengths
hold for whatever blocks it meets."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest
import zlib

import png_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ditherpie_hip_png.h")
CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
DP_OK, DP_EINVAL, DP_EUNSUPPORTED, DP_EWORKSPACE = 0, 1, 2, 5
N_RANDOM = 200

# size of the device's (= the host statement's) stream / zlib level 1 with Z_FIXED, photo-like 512 x 768 plane at the default
# seg_bytes, as measured when the encoder was written
RECORDED = {16: 1.0983, 256: 0.9918}


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


def _check_case(be, name, planes, depth, seg):
    """zlib, the walker and the rules of the header on every frame; -> the streams"""
    n, h, w = planes.shape
    streams = be.png_deflate_host(planes, depth, seg)
    assert len(streams) == n
    F = pr.filtered_size(h, w, depth)
    s = min(seg, F)
    for f, stream in enumerate(streams):
        want = pr.filtered(planes[f], depth)
        assert zlib.decompress(stream) == want, name
        assert len(stream) <= pr.bound_bytes(h, w, depth, seg), name
        got, blocks = pr.walk(stream)
        assert got == want, name
        segs = pr.segments_of(blocks)
        assert len(segs) == pr.n_segments(F, seg), name
        for j, (b, _) in enumerate(segs):
            assert (b["out0"], b["out1"]) == (j * s, min(F, (j + 1) * s)), name
            assert b["reach"] is None or b["reach"] >= b["out0"], (name, "a match reaches before its segment")
            assert b["maxlen"] <= 15 and b["maxcl"] <= 7, name
            last = j == len(segs) - 1
            tokens = pr.greedy_tokens(want[b["out0"]:b["out1"]])
            sizes = pr.segment_sizes(tokens, b["out1"] - b["out0"], last)
            assert b["type"] == pr.smallest_type(sizes), (name, j, sizes)
            if b["type"] != pr.STORED:
                assert b["tokens"] == tokens, (name, j)
            end = -(-b["bit1"] // 8) if last else segs[j + 1][0]["bit0"] // 8
            assert sizes[b["type"]] == end - b["bit0"] // 8, (name, j)   # the bytes the rule counted are the bytes written
    return streams


def _pillow(data, planes_f, palette, depth):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "P" and im.size == (planes_f.shape[1], planes_f.shape[0])
    kinds = pr.chunks_of(data)
    assert [k for k, _ in kinds][:2] == [b"IHDR", b"PLTE"] and kinds[-1] == (b"IEND", b"") and all(k == b"IDAT" for k, _ in kinds[2:-1])
    assert kinds[0][1][8:] == bytes([depth, 3, 0, 0, 0]) and len(kinds[1][1]) == 3 * len(palette)
    assert np.array_equal(np.asarray(im.convert("RGB")), np.asarray(palette, np.uint8)[planes_f])


def test_named_cases(be):
    rs = np.random.RandomState(3)
    seen = set()
    for name, planes, depth, seg in pr.named_cases():
        streams = _check_case(be, name, planes, depth, seg)
        palette = rs.randint(0, 256, (1 << depth, 3))
        masked = planes & ((1 << depth) - 1)
        for f, stream in enumerate(streams):
            _pillow(pr.container(planes.shape[2], planes.shape[1], depth, palette, stream), masked[f], palette, depth)
            seen |= {b["type"] for b in pr.walk(stream)[1] if b["out1"] > b["out0"]}
    assert seen == {pr.STORED, pr.FIXED}


def test_what_the_named_cases_are_there_for(be):
    cases = {name: (planes, depth, seg) for name, planes, depth, seg in pr.named_cases()}

    def blocks(name):
        planes, depth, seg = cases[name]
        return [b for b, _ in pr.segments_of(pr.walk(be.png_deflate_host(planes, depth, seg)[0])[1])], pr.filtered_size(*planes.shape[1:], depth)
    b, F = blocks("flat")
    assert any(t == (258, 1) for t in b[0]["tokens"])                  # runs longer than 258 at distance 1
    b, F = blocks("flat to the segment end")
    assert F == 512 and len(b) == 1 and isinstance(b[0]["tokens"][-1], tuple)   # the last match ends at the segment's last byte
    b, F = blocks("distance close to the segment")
    assert max(t[1] for t in b[0]["tokens"] if isinstance(t, tuple)) == 1984 and F == 2048 and len(b) == 1
    b, F = blocks("distance close to 32768")
    far = max((t for t in b[0]["tokens"] if isinstance(t, tuple)), key=lambda t: t[1])
    assert F == 32768 and len(b) == 1 and b[0]["type"] == pr.FIXED
    assert far[1] == 32512 and 227 <= far[0] <= 257                    # 13 extra distance bits, 5 extra length bits: a 31-bit token
    assert b[0]["tokens"][-1] == far                                   # ... that ends at the segment's last byte
    for name, runs in pr.CODE_LENGTH_RUNS.items():
        b, F = blocks(name)
        assert len(b) == 1 and all(not isinstance(t, tuple) for t in b[0]["tokens"]), name
        assert pr.runs_of_symbols(b[0]["tokens"]) == runs, name        # the alphabet the segment was made for
        assert sorted(b[0]["tokens"]).count(0) == 1 and len(set(b[0]["tokens"])) == len(b[0]["tokens"])   # equal counts
    lens = sorted(n for runs in pr.CODE_LENGTH_RUNS.values() for kind, n in runs[1:-1] if kind == "a")
    assert [n for n in (3, 6, 7, 10, 11, 138, 139) if n in lens] == [3, 6, 7, 10, 11, 138, 139]
    reps = {n for runs in pr.CODE_LENGTH_RUNS.values() for kind, n in runs if kind == "p"}
    assert {3, 6, 7, 10, 11, 138, 139} <= reps
    b, F = blocks("period of half a 8 KiB segment")
    assert max(t[1] for t in b[0]["tokens"] if isinstance(t, tuple)) >= 4000
    b, F = blocks("noise 256")
    assert all(x["type"] == pr.STORED for x in b) and len(b) == 2
    b, F = blocks("20-byte segment")
    assert F == 20 and b[0]["type"] == pr.FIXED
    b, F = blocks("all literals")
    assert all(not isinstance(t, tuple) for t in b[0]["tokens"])
    b, F = blocks("one distance")
    assert len({t[1] for t in b[0]["tokens"] if isinstance(t, tuple)}) == 1
    b, F = blocks("one distinct literal")
    assert {t for t in b[0]["tokens"] if not isinstance(t, tuple)} == {0}
    b, F = blocks("fibonacci counts")
    assert F == 32768 and len(b) == 1
    b, F = blocks("last segment of 1 byte")
    assert b[-1]["out1"] - b[-1]["out0"] == 1
    b, F = blocks("last segment of 2 bytes")
    assert b[-1]["out1"] - b[-1]["out0"] == 2
    b, F = blocks("seg == F")
    assert len(b) == 1 and F == 512
    b, F = blocks("boundary in mid-row")
    assert 300 % pr.row_bytes(99, 4) != 0 and len(b) == -(-F // 300)


def test_random_cases(be):
    cases = pr.random_cases(N_RANDOM)
    assert len({(c[2], c[3]) for c in cases}) > 20
    for name, planes, depth, seg in cases:
        n, h, w = planes.shape
        for f, stream in enumerate(be.png_deflate_host(planes, depth, seg)):
            assert zlib.decompress(stream) == pr.filtered(planes[f], depth), name
            assert len(stream) <= pr.bound_bytes(h, w, depth, seg), name
    for name, planes, depth, seg in cases[:25]:                        # the walker's rules on some of them
        _check_case(be, name, planes, depth, seg)


def test_segments_are_independent(be):
    rs = np.random.RandomState(5)
    a = pr.content("photo", rs, 1, 60, 90, 16)[0]
    b = a.copy()
    b[:5] = rs.randint(0, 16, (5, 90))                                 # rows of 46 bytes: 230 bytes, inside segment 0 of 512
    sa, sb = (be.png_deflate_host(x, 4, 512)[0] for x in (a, b))
    wa, wb = (pr.segments_of(pr.walk(s)[1]) for s in (sa, sb))
    assert sa != sb and len(wa) == len(wb) > 3
    ta, tb = wa[1][0]["bit0"] // 8, wb[1][0]["bit0"] // 8
    assert sa[ta:-4] == sb[tb:-4]                                      # from segment 1's data on, up to the Adler-32
    assert all(x["reach"] is None or x["reach"] >= x["out0"] for x, _ in wa + wb)


def test_out_of_range_indices_are_masked(be):
    rs = np.random.RandomState(6)
    for d in pr.DEPTHS:
        p = rs.randint(0, 256, (2, 9, 21)).astype(np.uint8)
        assert be.png_deflate_host(p, d, 256) == be.png_deflate_host(p & ((1 << d) - 1), d, 256)
        assert zlib.decompress(be.png_deflate_host(p, d, 256)[1]) == pr.filtered(p[1], d)


# ------------------------------------------------------------------------------------------------------------ sizes
def _zfixed1(data):
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    return co.compress(data) + co.flush()


def test_flat_plane_is_a_twentieth(be):
    p = np.full((256, 256), 9, np.uint8)
    F = pr.filtered_size(256, 256, 8)
    assert len(be.png_deflate_host(p, 8, None)[0]) * 20 <= F
    assert len(zlib.compress(pr.filtered(p, 8), 1)) * 20 <= F          # and so is zlib level 1


@pytest.mark.parametrize("k", [16, 256])
def test_size_against_zlib_fixed_level_1(be, k):
    """Stored and fixed blocks only, so the yardstick is zlib level 1 restricted to fixed codes (Z_FIXED): the same
    algorithmic class (single probe, greedy) with the same code."""
    assert be.PNG_SEG_BYTES == pr.SEG_DEFAULT
    plane, d = pr.photo_plane(k), pr.depth_of(k)
    raw = pr.filtered(plane, d)
    ours = be.png_deflate_host(plane, d, None)[0]
    assert zlib.decompress(ours) == raw
    ratio = len(ours) / len(_zfixed1(raw))
    print(f"k={k}: {len(ours)} bytes, {len(ours) / len(raw):.4f} of the filtered size, {ratio:.4f} of zlib Z_FIXED level 1, "
          f"{len(ours) / len(zlib.compress(raw, 1)):.4f} of zlib level 1")
    assert ratio <= RECORDED[k] + 0.02
    assert ratio <= 1.15


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_helpers_and_refusals(L, be):
    for h, w, d, seg in [(1, 1, 1, 256), (5, 9, 2, 300), (100, 333, 4, 8192), (2160, 3840, 8, 32768), (7, 7, 8, 32768)]:
        F = pr.filtered_size(h, w, d)
        assert L.dp_png_filtered_bytes(h, w, d) == F
        assert L.dp_png_deflate_bound_bytes(h, w, d, seg) == pr.bound_bytes(h, w, d, seg) == 2 + F + 10 * pr.n_segments(F, seg) + 4
        one, three = (L.dp_png_deflate_workspace_bytes(n, h, w, d, seg) for n in (1, 3))
        assert one >= min(seg, F) + 10 and three >= 3 * (one - 16) and L.dp_png_deflate_workspace_bytes(0, h, w, d, seg) == 0
    bad = [(0, 4, 8, 256), (4, 0, 8, 256), (-1, 4, 8, 256), (4, 4, 3, 256), (4, 4, 0, 256), (4, 4, 16, 256), (4, 4, 8, 255), (4, 4, 8, 32769),
           (4, 4, 8, 0), (1 << 16, 1 << 15, 8, 256), (46341, 46341, 8, 256)]
    for h, w, d, seg in bad:
        assert L.dp_png_deflate_bound_bytes(h, w, d, seg) == 0 and L.dp_png_deflate_workspace_bytes(1, h, w, d, seg) == 0, (h, w, d, seg)
    assert L.dp_png_filtered_bytes(1 << 16, 1 << 15, 8) == 0 and L.dp_png_filtered_bytes(4, 4, 5) == 0
    assert L.dp_png_filtered_bytes(1 << 15, (1 << 16) - 2, 8) == (1 << 31) - (1 << 15)         # just below 2^31
    assert L.dp_png_deflate_workspace_bytes(-1, 4, 4, 8, 256) == 0

    p = np.zeros((2, 4, 4), np.uint8)
    stride = L.dp_png_deflate_bound_bytes(4, 4, 8, 256)
    out, sizes = np.full((2, stride), 0xAB, np.uint8), np.full(2, -7, np.int64)
    ok = [_ptr(p), 2, 4, 4, 8, 256, _ptr(out), stride, _ptr(sizes)]

    def host(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[dict(planes=0, n=1, h=2, w=3, depth=4, seg=5, out=6, stride=7, sizes=8)[key]] = v
        return L.dp_png_deflate_host_u8(*a)
    for kw in (dict(planes=None), dict(out=None), dict(sizes=None), dict(n=-1), dict(h=0), dict(w=0), dict(depth=3), dict(seg=255), dict(seg=32769),
               dict(stride=stride - 1), dict(h=1 << 16, w=1 << 15)):
        assert host(**kw) == DP_EINVAL and b"dp_png_deflate_host_u8" in L.dp_last_error(), kw
    assert host(n=0) == DP_OK
    assert (out == 0xAB).all() and (sizes == -7).all()                  # nothing was touched
    assert host() == DP_OK and sizes.tolist() == [len(s) for s in be.png_deflate_host(p, 8, 256)]

    # the device entry point refuses before any HIP call: no device is needed to see it
    dev = [0x1000, 2, 4, 4, 8, 256, 0x2000, stride, 0x3000, 0x4000, 1 << 20, None]

    def device(**kw):
        a = list(dev)
        for key, v in kw.items():
            a[dict(planes=0, n=1, h=2, w=3, depth=4, seg=5, out=6, stride=7, sizes=8, ws=9, need=10)[key]] = v
        rc = L.dp_png_deflate_encode_u8(*a)
        assert b"dp_png_deflate_encode_u8" in L.dp_last_error()
        return rc
    for kw in (dict(planes=None), dict(out=None), dict(sizes=None), dict(ws=None), dict(n=-1), dict(h=0), dict(w=-3), dict(depth=7), dict(seg=100),
               dict(seg=40000), dict(stride=stride - 1), dict(sizes=0x3004), dict(ws=0x4008), dict(h=1 << 16, w=1 << 15)):
        assert device(**kw) == DP_EINVAL, kw
    assert device(need=L.dp_png_deflate_workspace_bytes(2, 4, 4, 8, 256) - 1) == DP_EWORKSPACE and device(need=0) == DP_EWORKSPACE
    assert device(n=65536, need=1 << 40) == DP_EUNSUPPORTED
    big = L.dp_png_deflate_bound_bytes(1 << 15, 1 << 15, 8, 256)
    assert device(n=65535, h=1 << 15, w=1 << 15, stride=big, need=1 << 60) == DP_EUNSUPPORTED   # 65535 frames of 2^22 segments
    assert L.dp_png_deflate_encode_u8(0x1000, 0, 4, 4, 8, 256, 0x2000, stride, 0x3000, 0x4000, 0, None) == DP_OK   # n == 0: a no-op


def test_wrapper_argument_checks(be):
    p = np.zeros((1, 4, 4), np.uint8)
    for depth, seg in ((3, None), (0, None), (8, 255), (8, 32769)):
        with pytest.raises(ValueError):
            be.png_deflate_host(p, depth, seg)
    with pytest.raises(ValueError):
        be.png_deflate_host(np.zeros((0, 4), np.uint8), 8)
    assert be.png_deflate_host(np.zeros((0, 4, 4), np.uint8), 8) == []
    assert [be.png_depth(k) for k in (1, 2, 3, 4, 5, 16, 17, 256)] == [1, 1, 2, 2, 4, 4, 8, 8]
    for k in (0, 257):
        with pytest.raises(ValueError):
            be.png_depth(k)
    assert be.png_deflate_stride(4, 4, 8, 256) == pr.bound_bytes(4, 4, 8, 256)


# ------------------------------------------------------------------------------------------------------------ container
def test_encode_png_with_the_host_encoder(tmp_path):
    from PIL import Image
    from dither_pie_amd import png
    rs = np.random.RandomState(8)
    for k in (2, 3, 16, 17, 256):
        palette = rs.randint(0, 256, (k, 3))
        planes = rs.randint(0, k, (3, 23, 37)).astype(np.uint8)
        files = png.encode_png(planes, palette, encoder="host")
        assert len(files) == 3
        for f, data in enumerate(files):
            _pillow(data, planes[f], palette, pr.depth_of(k))
            stream = b"".join(body for kind, body in pr.chunks_of(data) if kind == b"IDAT")
            assert data == pr.container(37, 23, pr.depth_of(k), palette, stream)
    one = png.encode_png(planes[0], palette, seg_bytes=256, encoder="host")
    assert len(one) == 1 and one[0] != files[0] and np.array_equal(np.asarray(Image.open(io.BytesIO(one[0])).convert("RGB")), palette[planes[0]].astype(np.uint8))
    assert png.write_png(str(tmp_path / "a.png"), planes[1], palette, encoder="host") == len(files[1])
    assert (tmp_path / "a.png").read_bytes() == files[1]
    paths = png.write_png_sequence(str(tmp_path / "frame_%05d.png"), planes, palette, start=4, encoder="host")
    assert [os.path.basename(p) for p in paths] == ["frame_00004.png", "frame_00005.png", "frame_00006.png"]
    assert [open(p, "rb").read() for p in paths] == files
    # a stream longer than an IDAT chunk is cut, and decodes the same
    cut = png.container(37, 23, 8, palette, stream, idat_bytes=100)
    assert sum(kind == b"IDAT" for kind, _ in pr.chunks_of(cut)) == -(-len(stream) // 100) > 1
    _pillow(cut, planes[2], palette, 8)


def test_encode_png_refusals(tmp_path):
    import torch
    from dither_pie_amd import png
    pal = np.zeros((4, 3), np.uint8)
    p = np.zeros((2, 5, 5), np.uint8)
    with pytest.raises(ValueError, match="256 colours"):
        png.encode_png(p, np.zeros((257, 3), np.uint8), encoder="host")
    with pytest.raises(ValueError, match="one-byte"):
        png.encode_png(p.astype(np.int16), pal, encoder="host")
    with pytest.raises(ValueError, match="one-byte"):
        png.encode_png(torch.zeros((2, 5, 5), dtype=torch.int16), pal, encoder="host")
    with pytest.raises(ValueError, match="CUDA"):
        png.encode_png(p, pal)                                          # the device encoder takes CUDA planes
    with pytest.raises(ValueError, match="CUDA"):
        png.encode_png(torch.zeros((2, 5, 5), dtype=torch.uint8), pal, encoder="device")
    with pytest.raises(ValueError, match="encoder"):
        png.encode_png(p, pal, encoder="zlib")
    with pytest.raises(ValueError):
        png.encode_png(p, np.zeros((4, 4), np.uint8), encoder="host")
    with pytest.raises(ValueError, match="one plane"):
        png.write_png(str(tmp_path / "x.png"), p, pal, encoder="host")
    assert not (tmp_path / "x.png").exists()
    assert png.encode_png(np.zeros((0, 5, 5), np.uint8), pal, encoder="host") == []


def test_process_video_pngs_refuses_before_anything_starts(tmp_path, monkeypatch):
    from dither_pie_amd import video_processor as v
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.scenes import Scene
    started = []
    monkeypatch.setattr(v.VideoProcessor, "_scan_decoded", lambda self, *a, **k: started.append(a))
    monkeypatch.setattr(v.VideoProcessor, "get_video_info", lambda self, *a, **k: started.append(a))
    d = ImageDitherer(4, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    pat = str(tmp_path / "f_%05d.png")
    many = [(i, i, i) for i in range(256)] + [(1, 2, 3)]
    for kw in (dict(max_frames=0), dict(seg_bytes=100), dict(seg_bytes=40000), dict(scene_palettes=[Scene(0, 5, None)]),
               dict(scene_palettes=[Scene(0, 5, many)]), dict(scene_palettes=[])):
        with pytest.raises(ValueError):
            v.VideoProcessor(devices=[0]).process_video_pngs("in.mp4", pat, d, **kw)
    with pytest.raises(ValueError, match="one device"):
        v.VideoProcessor(devices=[0, 1]).process_video_pngs("in.mp4", pat, d)
    with pytest.raises(ValueError, match="frame number"):
        v.VideoProcessor(devices=[0]).process_video_pngs("in.mp4", str(tmp_path / "same.png"), d)
    with pytest.raises(ValueError, match="256"):
        v.VideoProcessor(devices=[0]).process_video_pngs("in.mp4", pat, ImageDitherer(257, DitherMode.BAYER, many))
    assert started == [] and list(tmp_path.iterdir()) == []


# ------------------------------------------------------------------------------------------------------------ sanitizers
def test_host_statement_under_the_sanitizers(be, tmp_path):
    """The stand-alone harness (csrc/host_sanitize.cpp, built with -fsanitize=address,undefined) runs png_deflate_encode on
    planes of exactly h * w bytes and prints the bytes the library's host statement gives."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    cases = [c for c in pr.named_cases() if c[1].size <= 40000][::3] + pr.random_cases(24, seed=12)
    with open(tmp_path / "cases.bin", "wb") as f:
        for _, planes, depth, seg in cases:
            n, h, w = planes.shape
            f.write(np.array([n, h, w, depth, seg], np.int32).tobytes() + planes.tobytes())
    r = subprocess.run([os.path.join(CSRC, "build", "host_asan"), "pngdeflate", str(tmp_path / "cases.bin"), str(len(cases))],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    want = [(c, k, s) for c, (_, planes, depth, seg) in enumerate(cases) for k, s in enumerate(be.png_deflate_host(planes, depth, seg))]
    assert len(lines) == len(want)
    for ln, (c, k, s) in zip(lines, want):
        assert (int(ln[1]), int(ln[2]), int(ln[3])) == (c, k, len(s)) and bytes.fromhex(ln[4]) == s, (c, k)


# ------------------------------------------------------------------------------------------------------------ the header
def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"\b(dp_\w+)\s*\(", text)


def test_header_exports_and_memory_matrix_agree():
    import importlib
    import sys
    from dither_pie_amd import _lib
    names = _header_functions()
    assert len(names) == len(set(names)) == 5
    assert sorted(names) == sorted(_lib.EXPORTS_PNG)
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
    assert not others & set(_lib.EXPORTS_PNG)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    mem = importlib.import_module("test_gpu_png_memory")
    device = {n for n in names if not n.endswith(("_bytes", "_host_u8"))}   # what takes device pointers
    assert set(mem.COVERAGE) | set(mem.EXCLUDED) == device and not set(mem.COVERAGE) & set(mem.EXCLUDED)
    for fn, tests in mem.COVERAGE.items():
        assert tests and all(callable(getattr(mem, t)) for t in tests), fn
    assert _lib.ABI_VERSION == 103 and _lib.load().dp_version() == 103          # additions: the revision is unchanged
    assert "#define DP_ABI_VERSION 103" in open(os.path.join(ROOT, "include", "ditherpie_hip.h")).read()
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes is not None
