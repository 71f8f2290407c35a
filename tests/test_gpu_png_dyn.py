"""GPU tier: dynamic-Huffman blocks on the device (include/ditherpie_hip_png_dyn.h).  backend.png_deflate(blocks="dynamic")
writes the bytes of the host statement (backend.png_deflate_host(blocks="dynamic"), itself judged by the Python restatement
of tests/png_dyn_ref.py, zlib, the walker and Pillow in tests/test_png_dyn_cpu.py), sizes included, on the named cases, the
cases the dynamic blocks were added for and random ones, alone and in batches of three at odd addresses, and on the
many-segment shapes; batching is invisible; the code construction on its own (backend.png_code_lengths) equals its host
twin up to the 15-bit limit; files written with blocks="dynamic" decode in Pillow to what the RGB routes give.
Runs on the product library.  No test here is meant to fault."""
import io
import zlib

import numpy as np
import pytest

import png_dyn_ref as dr
import png_ref as pr

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
    payload, sizes = be.png_deflate(_at_offset(T, planes, off), depth, seg, blocks="dynamic")
    assert payload.dtype == T.uint8 and sizes.dtype == T.int64
    assert payload.shape == (len(planes), be.png_deflate_stride(planes.shape[1], planes.shape[2], depth, seg))
    sizes = sizes.cpu().tolist()
    payload = payload.cpu().numpy()
    return [payload[f, :n].tobytes() for f, n in enumerate(sizes)]


def _host(be, planes, depth, seg):
    return be.png_deflate_host(planes, depth, seg, blocks="dynamic")


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


def _types(stream):
    return {b["type"] for b, _ in pr.segments_of(dr.walk(stream)[1])}


# ---------------------------------------------------------------------------------------------------- encoder bytes
def test_encoder_equals_the_host_statement_on_the_named_and_new_cases(T, be):
    rs = np.random.RandomState(41)
    seen = set()
    for name, planes, depth, seg in pr.named_cases() + dr.new_cases():
        got = _encode(T, be, planes, depth, seg)
        _same(got, _host(be, planes, depth, seg), name)
        seen |= _types(got[0])
        three = _three(planes, rs)
        got = _encode(T, be, three, depth, seg, off=3)
        _same(got, _host(be, three, depth, seg), name + " x3")
        assert zlib.decompress(got[1]) == pr.filtered(three[1], depth), name
    assert seen == {pr.STORED, pr.FIXED, pr.DYNAMIC}


def test_encoder_on_random_cases(T, be):
    rs = np.random.RandomState(42)
    for i, (name, planes, depth, seg) in enumerate(pr.random_cases(N_RANDOM, seed=13)):
        _same(_encode(T, be, planes[:1], depth, seg, off=i % 4), _host(be, planes[:1], depth, seg), name)
        three = _three(planes, rs)
        _same(_encode(T, be, three, depth, seg, off=(i + 1) % 4), _host(be, three, depth, seg), name + " x3")


@pytest.mark.parametrize("n, h, w, depth, why", [
    (10, 300, 300, 8, "353 segments a frame, 3530 in the call: the segment kernel's waves take a second segment on the LDS (histograms, "
                      "codes, builder scratch) and the token area they used"),
    (1, 520, 520, 8, "1059 segments in one frame: the pack kernel strides over them"),
    (3, 700, 1001, 1, "depth 1 over many rows: 349 segments a frame with 2.03 rows each")])
def test_many_segments_equal_the_host_statement(T, be, n, h, w, depth, why):
    rs = np.random.RandomState(25)
    k = 1 << min(depth, 4)
    planes = np.concatenate([pr.content(pr.KINDS[f % 4], rs, 1, h, w, k if f % 2 else 1 << depth) for f in range(n)])
    F = pr.filtered_size(h, w, depth)
    assert pr.n_segments(F, 256) > (1024 if n == 1 else 64) and (n != 10 or n * pr.n_segments(F, 256) > 3072), why
    got = _encode(T, be, planes, depth, 256, off=1)
    _same(got, _host(be, planes, depth, 256), why)
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
        assert pr.DYNAMIC in set().union(*(_types(s) for s in together))


def test_out_of_range_indices_are_masked(T, be):
    rs = np.random.RandomState(24)
    p = rs.randint(0, 256, (2, 19, 45)).astype(np.uint8)
    for depth in pr.DEPTHS:
        got = _encode(T, be, p, depth, 256)
        assert got == _encode(T, be, p & ((1 << depth) - 1), depth, 256) == _host(be, p, depth, 256)


def test_argument_checks_of_the_wrapper(T, be):
    p = T.zeros((2, 4, 4), dtype=T.uint8, device="cuda")
    for blocks in ("stored", None, "Dynamic", 2):
        with pytest.raises(ValueError, match="blocks"):
            be.png_deflate(p, 8, blocks=blocks)
    payload, sizes = be.png_deflate(p[:0], 8, blocks="dynamic")
    assert payload.shape[0] == 0 and sizes.numel() == 0
    assert be.png_deflate(p, 8, blocks="fixed")[1].tolist() == be.png_deflate(p, 8)[1].tolist()
    with pytest.raises(ValueError):
        be.png_code_lengths(T.zeros((2, 300), dtype=T.int32, device="cuda"), 15)
    with pytest.raises(ValueError):
        be.png_code_lengths(T.zeros((2, 30), dtype=T.int32, device="cuda"), 4)
    with pytest.raises(ValueError):
        be.png_code_lengths(np.zeros((2, 30), np.int32), 15)
    assert be.png_code_lengths(T.zeros((0, 30), dtype=T.int32, device="cuda"), 15).shape == (0, 30)


# ---------------------------------------------------------------------------------------------------- the code construction
def test_code_lengths_equal_the_host_twin(T, be):
    cases = dr.builder_inputs() + [c for L in (15, 9, 7) for c in dr.random_histograms(L)]
    over = 0
    for (m, L) in sorted({(len(c), L) for _, c, L in cases}):
        group = [(name, c) for name, c, l in cases if (len(c), l) == (m, L)]
        counts = np.array([c for _, c in group], np.int64)
        want = be.png_code_lengths_host(counts, L)
        got = be.png_code_lengths(T.from_numpy(counts).cuda(), L).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == counts.shape
        for i, (name, c) in enumerate(group):
            assert got[i].tolist() == want[i].tolist(), name
            assert int(got[i].max()) <= L and abs(dr.kraft(got[i].tolist()) - 1.0) < 1e-12, name
            over += int(got[i].max()) == L
    assert over >= 10                                                   # the limit was met, at 15 bits among others
    fib = be.png_code_lengths(T.tensor(dr.fibonacci(21), device="cuda"), 15).cpu().tolist()
    assert fib == dr.code_lengths(dr.fibonacci(21), 15) and max(fib) == 15 and fib.count(15) > 2
    many = np.tile(np.array(dr.fibonacci(21) + [0] * 9, np.int64), (5000, 1))        # more histograms than workgroups: grid stride
    got = be.png_code_lengths(T.from_numpy(many).cuda(), 15).cpu().numpy()
    assert (got == got[0]).all() and got[0, :21].tolist() == fib and not got[0, 21:].any()


# ---------------------------------------------------------------------------------------------------- through the layers
def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "P"
    return im, np.asarray(im.convert("RGB")).copy()


def _stream_of(data):
    return b"".join(body for kind, body in pr.chunks_of(data) if kind == b"IDAT")


@pytest.mark.parametrize("k", [16, 256])
def test_encode_png_decodes_to_the_palette_of_the_planes(T, tmp_path, k):
    from dither_pie_amd import png
    rs = np.random.RandomState(31)
    palette = rs.randint(0, 256, (k, 3)).astype(np.uint8)
    planes = np.concatenate([pr.content("photo", rs, 2, 96, 130, k), pr.content("noise", rs, 1, 96, 130, k)])
    dev = T.from_numpy(planes).cuda()
    files = png.encode_png(dev, palette, blocks="dynamic")
    assert len(files) == 3 and files == png.encode_png(planes, palette, encoder="host", blocks="dynamic")
    fixed = png.encode_png(dev, palette)
    for f, data in enumerate(files):
        im, got = _decode(data)
        assert im.size == (130, 96) and np.array_equal(got, palette[planes[f]])
        assert len(data) <= len(fixed[f])
    assert pr.DYNAMIC in _types(_stream_of(files[0])) and len(files[0]) < len(fixed[0])
    assert png.write_png(str(tmp_path / "s.png"), dev[1], palette, blocks="dynamic") == len(files[1])
    assert (tmp_path / "s.png").read_bytes() == files[1]
    paths = png.write_png_sequence(str(tmp_path / "frame_%05d.png"), dev, palette, blocks="dynamic")
    assert [open(p, "rb").read() for p in paths] == files
    with pytest.raises(ValueError, match="blocks"):
        png.encode_png(dev, palette, blocks="best")


@pytest.mark.parametrize("mode", ["bayer", "fs"])
@pytest.mark.parametrize("k", [16, 256])
def test_apply_dithering_png_decodes_to_apply_dithering(T, mode, k):
    from PIL import Image
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    rs = np.random.RandomState(32)
    y, x = np.mgrid[0:75, 0:101]
    img = Image.fromarray(np.stack([(x * 3) % 256, (y * 4) % 256, (x + y) % 256], axis=-1).astype(np.uint8), "RGB")
    pal = sorted({tuple(int(v) for v in c) for c in rs.randint(0, 256, (2 * k, 3))})[:k]
    d = (ImageDitherer(k, DitherMode.BAYER, pal, dither_params={"size": "4x4"}) if mode == "bayer" else
         ImageDitherer(k, DitherMode.ERROR_DIFFUSION, pal, dither_params={"variant": "floyd_steinberg"}))
    want = np.asarray(d.apply_dithering(img))
    data = d.apply_dithering_png(img, blocks="dynamic")
    im, got = _decode(data)
    assert isinstance(data, bytes) and im.size == (101, 75) and np.array_equal(got, want)
    assert pr.chunks_of(data)[0][1][8] == pr.depth_of(k)
    assert len(data) <= len(d.apply_dithering_png(img))
    if k == 16:                                                         # few byte values: a dynamic block is certain to win
        assert pr.DYNAMIC in _types(_stream_of(data))
    with pytest.raises(ValueError, match="blocks"):
        d.apply_dithering_png(img, blocks="huffman")


def test_process_frames_png_decodes_to_process_frames(T):
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.video_processor import process_frames, process_frames_png
    rs = np.random.RandomState(33)
    frames = T.from_numpy(rs.randint(0, 256, (3, 90, 120, 3)).astype(np.uint8)).cuda()
    d = ImageDitherer(5, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 200, 30), (30, 30, 200)], dither_params={"size": "4x4"})
    want = process_frames(frames, d, "regular", 48, 3).cpu().numpy()
    files = process_frames_png(frames, d, "regular", 48, 3, blocks="dynamic")
    assert len(files) == 3 and [len(f) for f in files] <= [len(f) for f in process_frames_png(frames, d, "regular", 48, 3)]
    for i, data in enumerate(files):
        assert np.array_equal(_decode(data)[1], want[i])
