"""CPU tier of the animated GIF output (include/ditherpie_hip_gif.h, dither_pie_amd/gif.py): Pillow judges the plain-Python
statement tests/gif_ref.py (every container it builds opens, and every frame decodes to palette[planes]); the library's host
statement (dp_gif_lzw_host_u8 through ctypes, and the `giflzw` subcommand of the stand-alone host_asan build) writes the bytes
of gif_ref on the named cases, the sub-block edges and 200 seeded random cases; the agreement of the header, the ctypes table
and the memory-discipline module (the rule tests/test_scenes_cpu.py keeps for the scene header); the refusals of the entry
points, which happen before any HIP call; GifWriter's container logic on the host encoder."""
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import gif_ref as gr
from conftest import ROOT

N_RANDOM = 200


# ---------------------------------------------------------------------------------------------------- shared references
@pytest.fixture(scope="module")
def cases():
    """[(name, planes, min_code_size, chunk_px, [image data per frame by gif_ref])]: computed once, left unchanged."""
    out = [(name, p, mcs, chunk) for name, p, mcs, chunk in gr.named_cases()]
    edges = gr.subblock_edge_cases()
    assert sorted(edges) == [254, 255, 256, 509, 510, 511], sorted(edges)     # found, not skipped
    out += [(f"edge_{d}", p, 8, chunk) for d, (p, chunk) in sorted(edges.items())]
    out += [(f"random_{s}",) + gr.random_case(s) for s in range(N_RANDOM)]
    return [(name, p, mcs, chunk, [gr.image_data(f.reshape(-1), mcs, chunk) for f in p]) for name, p, mcs, chunk in out]


@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _host(lib, planes, mcs, chunk, stride=None):
    n, h, w = planes.shape
    stride = int(lib.dp_gif_lzw_bound_bytes(h, w, chunk)) if stride is None else stride
    out = np.full((n, stride), 0xA5, np.uint8)
    sizes = np.zeros(n, np.int64)
    p = np.ascontiguousarray(planes)
    rc = lib.dp_gif_lzw_host_u8(p.ctypes.data, n, h, w, mcs, chunk, out.ctypes.data, stride, sizes.ctypes.data)
    assert rc == 0, lib.dp_last_error()
    return [out[f, :sizes[f]].tobytes() for f in range(n)], stride


# ---------------------------------------------------------------------------------------------------- Pillow judges gif_ref
def _decode(data):
    im = Image.open(io.BytesIO(data))
    frames = []
    for i in range(im.n_frames):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return im, frames


def _palette(rs, k):
    pal = rs.permutation(256 * 256)[:k]                                 # distinct colours: a wrong index cannot hide
    return np.stack([pal & 0xFF, pal >> 8, (pal * 7) & 0xFF], axis=1).astype(np.uint8)


@pytest.mark.parametrize("k, h, w, chunk, kind, delta", [
    (2, 5, 7, 3, "noise", False), (16, 37, 53, 1, "tile", False), (16, 37, 53, 64, "tile", True), (256, 64, 70, 1000, "noise", True),
    (255, 33, 129, 4096, "tile", True), (3, 200, 200, None, "noise", False), (256, 96, 96, None, "noise", False), (4, 1, 1, 5, "noise", True),
    (16, 5, 5, 8, "noise", True), (16, 40, 40, 512, "flat", True)])
def test_pillow_decodes_what_gif_ref_builds(k, h, w, chunk, kind, delta):
    rs = np.random.RandomState(k * 1000 + h)
    planes = gr.content(kind, rs, 3, h, w, k)
    planes[2] = planes[1]                                               # a repeated frame: all transparent under delta
    pal = _palette(rs, k)
    frames = gr.clip_frames(planes, [pal] * 3, delta)
    if delta and k <= 255:
        assert frames[2][2] == k and (frames[2][0] == k).all() and frames[0][2] is None
        if k == 255:
            assert frames[1][2] == 255
    else:
        assert all(t is None for _, _, t in frames)                     # K = 256: no index is left, frames go out whole
    for fps, want_ms in ((25, 40), (30, 30), (100, 20), (7, 140)):
        data = gr.container(frames, w, h, fps, loop=3 if fps == 7 else 0, chunk_px=chunk)
        im, got = _decode(data)
        assert im.n_frames == 3 and im.info["duration"] == want_ms and im.info["loop"] == (3 if fps == 7 else 0)
        for i in range(3):
            assert np.array_equal(got[i], pal[planes[i]]), (k, h, w, chunk, i)
        if h * w > 5000:
            break                                                       # (the timing fields do not depend on the pixels)


def test_pillow_decodes_a_three_scene_clip_with_local_tables():
    rs = np.random.RandomState(77)
    ks, lengths = (4, 16, 200), (3, 2, 4)
    pals = [_palette(rs, k) for k in ks]
    planes = np.concatenate([gr.content("tile", rs, n, 30, 41, k) for k, n in zip(ks, lengths)])
    per_frame = [pals[s] for s, n in enumerate(lengths) for _ in range(n)]
    frames = gr.clip_frames(planes, per_frame, True)
    assert [t for _, _, t in frames] == [None, 4, 4, None, 16, None, 200, 200, 200]      # the delta starts over at a palette change
    data = gr.container(frames, 41, 30, 25, chunk_px=100)
    assert data.count(b"\x2c" + struct.pack("<HHHH", 0, 0, 41, 30)) >= 9
    im, got = _decode(data)
    assert im.n_frames == 9
    for i in range(9):
        assert np.array_equal(got[i], per_frame[i][planes[i]]), i


# ---------------------------------------------------------------------------------------------------- host statement = gif_ref
def test_host_entry_point_writes_the_bytes_of_gif_ref(lib, cases):
    for name, planes, mcs, chunk, want in cases:
        got, stride = _host(lib, planes, mcs, chunk)
        assert got == want, name
        assert stride == gr.bound_bytes(planes.shape[1], planes.shape[2], chunk) and all(len(b) <= stride for b in want), name


def test_sub_block_framing_at_the_edges(lib, cases):
    seen = set()
    for name, planes, mcs, chunk, want in cases:
        if not name.startswith("edge_"):
            continue
        d = int(name[5:])
        blob = _host(lib, planes, mcs, chunk)[0][0]
        assert blob == want[0] and blob[0] == 8
        full, rest = divmod(d, 255)
        at = 1
        for _ in range(full):
            assert blob[at] == 255
            at += 256
        if rest:
            assert blob[at] == rest
            at += 1 + rest
        assert at == len(blob) - 1 and blob[at] == 0                    # no empty block in front of the terminator
        assert len(blob) == 1 + d + full + (1 if rest else 0) + 1
        seen.add(d)
    assert seen == {254, 255, 256, 509, 510, 511}


def test_host_statement_under_the_sanitizers(cases, tmp_path):
    csrc = os.path.join(ROOT, "dither_pie_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "host_asan"])
    f = tmp_path / "cases.bin"
    with open(f, "wb") as out:
        for name, planes, mcs, chunk, want in cases:
            n, h, w = planes.shape
            out.write(struct.pack("<iiiiq", n, h, w, mcs, chunk) + np.ascontiguousarray(planes).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "host_asan"), "giflzw", str(f), str(len(cases))], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == sum(len(c[1]) for c in cases)
    at = 0
    for ci, (name, planes, mcs, chunk, want) in enumerate(cases):
        for k, blob in enumerate(want):
            tag, c, fr, size, hexed = lines[at].split(" ")
            assert (tag, int(c), int(fr), int(size)) == ("frame", ci, k, len(blob)) and bytes.fromhex(hexed) == blob, name
            at += 1


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_functions():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_gif.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        found[m.group(1)] = bool(re.search(r"\w+_dev\b", m.group(2)))
    return found


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_gif_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert len(found) == 5 and set(found) == set(_lib.EXPORTS_GIF), set(found) ^ set(_lib.EXPORTS_GIF)
    assert not set(_lib.EXPORTS_GIF) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE))
    with_dev = {n for n, d in found.items() if d}
    assert with_dev == {"dp_index_delta_u8", "dp_gif_lzw_encode_u8"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib
    L = _lib.load()
    for name in _lib.EXPORTS_GIF:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: gif.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_GIF:
            assert re.search(rf"\bT {name}\b", sym), (path, name)


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
def _refused(lib, rc, code, *words):
    msg = lib.dp_last_error().decode()
    assert rc == code, (rc, msg)
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                # (the product library spells out no status name)
    for w in words:
        assert w in msg, (w, msg)


def test_delta_refusals(lib):
    fn = "dp_index_delta_u8"
    ok = dict(planes=0x1000001, n=3, n_px=20, prev=0x2000003, has=1, t=16, out=0x3000005, changed=0x4000008)   # never dereferenced
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_index_delta_u8(v["planes"], v["n"], v["n_px"], v["prev"], v["has"], v["t"], v["out"], v["changed"], None)
    for bad in (dict(planes=None), dict(prev=None), dict(out=None), dict(changed=None), dict(n=-1), dict(n_px=0), dict(n_px=-5), dict(t=-1), dict(t=256),
                dict(t=1000), dict(changed=0x4000004), dict(changed=0x4000001), dict(prev=None, has=0)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for bad in (dict(out=0x1000001), dict(out=0x1000001 + 59), dict(out=0x1000001 - 59), dict(out=0x2000003), dict(out=0x2000003 - 59),
                dict(prev=0x1000001 + 40), dict(planes=0x2000003 - 10)):
        _refused(lib, call(**bad), 1, fn, "in-place")                   # the planes, the carried plane and out overlap
    for bad in (dict(n=65536), dict(n=2 ** 31 - 1)):
        _refused(lib, call(**bad), 2, fn, "65535")                      # DP_EUNSUPPORTED
    assert call(n=0) == 0 and call(n=0, has=0) == 0                     # nothing to do is not an error, and launches nothing


def test_encoder_refusals(lib):
    fn = "dp_gif_lzw_encode_u8"
    bound = lib.dp_gif_lzw_bound_bytes(9, 11, 16)
    need = lib.dp_gif_lzw_workspace_bytes(3, 9, 11, 16)
    assert bound > 0 and need > 0
    ok = dict(planes=0x1000001, n=3, h=9, w=11, mcs=4, chunk=16, out=0x3000005, stride=bound, sizes=0x4000008, ws=0x5000010, ws_bytes=need)
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_gif_lzw_encode_u8(v["planes"], v["n"], v["h"], v["w"], v["mcs"], v["chunk"], v["out"], v["stride"], v["sizes"], v["ws"],
                                        v["ws_bytes"], None)
    for bad in (dict(planes=None), dict(out=None), dict(sizes=None), dict(ws=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(h=65536, w=32768),
                dict(mcs=1), dict(mcs=9), dict(mcs=0), dict(chunk=0), dict(chunk=-4), dict(stride=bound - 1), dict(stride=0), dict(stride=-1),
                dict(sizes=0x4000004), dict(ws=0x5000008), dict(ws=0x5000001)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    _refused(lib, call(ws_bytes=need - 1), 5, fn, "workspace")          # DP_EWORKSPACE
    _refused(lib, call(ws_bytes=0), 5, fn, "workspace")
    big = lib.dp_gif_lzw_bound_bytes(9, 11, 1)
    _refused(lib, call(n=65536, ws_bytes=2 ** 40), 2, fn, "65535")      # DP_EUNSUPPORTED
    _refused(lib, call(n=65535, h=256, w=256, chunk=1, stride=lib.dp_gif_lzw_bound_bytes(256, 256, 1), ws_bytes=2 ** 50), 2, fn, "2^31 chunks")
    assert big > bound
    assert call(n=0) == 0 and call(n=0, ws_bytes=lib.dp_gif_lzw_workspace_bytes(0, 9, 11, 16)) == 0
    fn = "dp_gif_lzw_host_u8"
    plane = np.zeros((1, 9, 11), np.uint8)
    out = np.zeros(bound, np.uint8)
    size = np.zeros(1, np.int64)
    def host(**kw):
        v = dict(dict(planes=plane.ctypes.data, n=1, h=9, w=11, mcs=4, chunk=16, out=out.ctypes.data, stride=bound, sizes=size.ctypes.data), **kw)
        return lib.dp_gif_lzw_host_u8(v["planes"], v["n"], v["h"], v["w"], v["mcs"], v["chunk"], v["out"], v["stride"], v["sizes"])
    for bad in (dict(planes=None), dict(out=None), dict(sizes=None), dict(n=-1), dict(h=0), dict(w=-1), dict(mcs=1), dict(mcs=9), dict(chunk=0),
                dict(stride=bound - 1)):
        _refused(lib, host(**bad), 1, fn, "bad argument")
    assert host(n=0) == 0 and host() == 0 and size[0] > 0


def test_bound_and_workspace_sizes(lib, cases):
    B, W = lib.dp_gif_lzw_bound_bytes, lib.dp_gif_lzw_workspace_bytes
    for bad in ((0, 5, 8), (5, 0, 8), (5, 5, 0), (-1, 5, 8), (65536, 32768, 8)):
        assert B(*bad) == 0 and W(1, *bad) == 0
    assert W(-1, 5, 5, 8) == 0
    for chunk in (1, 3, 64, 4096, 2 ** 40):
        last = 0
        for side in (1, 2, 3, 7, 8, 9, 63, 64, 65, 100, 333, 1080):     # monotone in the frame's size
            b = B(side, side + 1, chunk)
            assert b > last and b == gr.bound_bytes(side, side + 1, chunk), (side, chunk)
            last = b
    assert [B(40, 50, c) for c in (1, 2, 10, 1999, 2000, 2001)] == sorted((B(40, 50, c) for c in (1, 2, 10, 1999, 2000, 2001)), reverse=True)
    assert B(40, 50, 2000) == B(40, 50, 10 ** 9)                        # a chunk beyond the frame is the frame
    assert W(2, 40, 50, 64) > W(1, 40, 50, 64) > 0 and W(1, 40, 50, 64) % 4 == 0
    for name, planes, mcs, chunk, want in cases:                        # the bound holds on everything the tests encode
        assert max(len(b) for b in want) <= B(planes.shape[1], planes.shape[2], chunk), name
    worst = np.arange(64 * 64, dtype=np.uint32)                         # no pair repeats early: close to a code per pixel
    worst = ((worst * 2654435761) >> 13).astype(np.uint8).reshape(1, 64, 64)
    for chunk in (1, 2, 7, 4096):
        got, stride = _host(lib, worst, 8, chunk)
        assert len(got[0]) <= stride and got[0] == gr.image_data(worst.reshape(-1), 8, chunk)


def test_out_of_range_indices_are_reduced_not_trusted(lib):
    planes = np.random.RandomState(4).randint(0, 256, (1, 20, 20)).astype(np.uint8)
    got, _ = _host(lib, planes, 3, 50)
    assert got[0] == gr.image_data((planes & 7).reshape(-1), 3, 50) == _host(lib, planes & 7, 3, 50)[0][0]


# ---------------------------------------------------------------------------------------------------- GifWriter on the host encoder
def _write(adds, w, h, fps, **kw):
    from dither_pie_amd.gif import GifWriter
    buf = io.BytesIO()
    with GifWriter(buf, w, h, fps, encoder="host", **kw) as g:
        for planes, pal, delta in adds:
            g.add(planes, pal, delta)
    return buf.getvalue()


def test_writer_container_equals_gif_ref_and_pillow_decodes_it():
    rs = np.random.RandomState(21)
    h, w = 24, 31
    pal_a, pal_b, pal_c = _palette(rs, 16), _palette(rs, 5), _palette(rs, 256)
    a = gr.content("tile", rs, 5, h, w, 16)
    a[3] = a[2]
    b = gr.content("tile", rs, 3, h, w, 5)
    c = gr.content("noise", rs, 2, h, w, 256)
    planes = np.concatenate([a, b, c, a[:2]])
    per_frame = [pal_a] * 5 + [pal_b] * 3 + [pal_c] * 2 + [pal_a] * 2
    for chunk in (50, None):
        kw = {} if chunk is None else dict(chunk_px=chunk)
        from dither_pie_amd import backend
        want = gr.container(gr.clip_frames(planes, per_frame, True), w, h, 30, 0, chunk or backend.GIF_CHUNK_PX)
        # the batch cut is invisible: a scene in one add, in two, frame by frame
        for cuts in ([(a, pal_a), (b, pal_b), (c, pal_c), (a[:2], pal_a)], [(a[:2], pal_a), (a[2:], pal_a), (b[:1], pal_b), (b[1:], pal_b), (c, pal_c), (a[:2], pal_a)],
                     [(p[None], q) for p, q in zip(planes, per_frame)]):
            assert _write([(p, q, True) for p, q in cuts], w, h, 30, **kw) == want, (chunk, len(cuts))
    im, got = _decode(want)
    assert im.n_frames == 12 and im.info["duration"] == 30 and im.info["loop"] == 0
    for i in range(12):
        assert np.array_equal(got[i], per_frame[i][planes[i]]), i
    # the table decision: the first palette is global, every other one local; coming back to the first one is global again
    heads = [m.start() for m in re.finditer(re.escape(b"\x2c" + struct.pack("<HHHH", 0, 0, w, h)), want)]
    flags = [want[at + 9] for at in heads][:12]
    assert flags == [0] * 5 + [0x80 | 2] * 3 + [0x80 | 7] * 2 + [0] * 2
    whole = gr.container(gr.clip_frames(planes, per_frame, False), w, h, 30, 0, 50)
    assert _write([(planes[i:i + 1], per_frame[i], False) for i in range(12)], w, h, 30, chunk_px=50) == whole
    assert len(whole) > len(want)                                       # (the deltas are what makes the file small)


def test_writer_delta_rules():
    from dither_pie_amd.gif import GifWriter
    rs = np.random.RandomState(22)
    h, w = 9, 13
    pal = _palette(rs, 255)
    p = gr.content("noise", rs, 4, h, w, 255)
    # delta=False frames still move the carried plane: the next delta frame compares with the frame before it
    got = _write([(p[:1], pal, True), (p[1:2], pal, False), (p[2:], pal, True)], w, h, 10)
    frames = gr.clip_frames(p, [pal] * 4, True)
    frames[1] = (p[1], pal, None)
    from dither_pie_amd import backend
    assert got == gr.container(frames, w, h, 10, 0, backend.GIF_CHUNK_PX)
    im, dec = _decode(got)
    assert all(np.array_equal(dec[i], pal[p[i]]) for i in range(4)) and im.info["duration"] == 100
    gce = [m.start() for m in re.finditer(re.escape(b"\x21\xf9\x04"), got)]
    assert [(got[at + 3] & 1, got[at + 6]) for at in gce][:4] == [(0, 0), (0, 0), (1, 255), (1, 255)]    # the transparent flag and index
    # K = 256: nothing is transparent, every frame whole
    pal256 = _palette(rs, 256)
    q = gr.content("noise", rs, 3, h, w, 256)
    q[1] = q[0]
    got = _write([(q, pal256, True)], w, h, 50)
    assert got == gr.container([(f, pal256, None) for f in q], w, h, 50, 0, backend.GIF_CHUNK_PX)
    assert _decode(got)[0].info["duration"] == 20
    # the delay rule
    from dither_pie_amd.gif import delay_cs
    assert [delay_cs(f) for f in (1000, 100, 60, 50, 40, 30, 29.97, 25, 24, 15, 10, 1, 0.5)] == [2, 2, 2, 2, 2, 3, 3, 4, 4, 7, 10, 100, 200]
    buf = io.BytesIO()
    g = GifWriter(buf, w, h, 25, loop=7, encoder="host")
    assert g.add(np.zeros((0, h, w), np.uint8), pal) == 0 and buf.getvalue() == b""
    g.close()
    assert buf.getvalue() == b"" and g.n_frames == 0                    # no frame, no file
    with pytest.raises(ValueError, match="closed"):
        g.add(p, pal)
    data = _write([(p[0], pal, True)], w, h, 25, loop=7)                # one plane [H,W]
    assert _decode(data)[0].info["loop"] == 7 and data[:6] == b"GIF89a" and data[-1:] == b"\x3b"


def test_writer_value_errors():
    import torch
    from dither_pie_amd.gif import GifWriter, write_gif
    h, w = 6, 8
    pal = [(0, 0, 0), (255, 255, 255), (9, 9, 9)]
    ok = np.zeros((2, h, w), np.uint8)
    g = GifWriter(io.BytesIO(), w, h, 25, encoder="host")
    for planes, palette in ((ok.astype(np.int16), pal), (torch.zeros((2, h, w), dtype=torch.int16), pal), (ok, [(1, 2, 3)] * 257), (ok[:, :5], pal),
                            (np.zeros((2, w, h), np.uint8), pal), (np.zeros((2, h, w, 1), np.uint8), pal), (ok, []), (ok, [(1, 2)]), (ok, [(1, 2, 300)])):
        with pytest.raises(ValueError):
            g.add(planes, palette)
    assert g.n_frames == 0 and g.add(torch.zeros((2, h, w), dtype=torch.uint8), pal) == 2
    d = GifWriter(io.BytesIO(), w, h, 25)                               # the device encoder: host input is refused by name, nothing falls back
    for planes in (ok, torch.zeros((2, h, w), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="CUDA"):
            d.add(planes, pal)
    for kw in (dict(width=0), dict(height=70000), dict(fps=0), dict(fps=-1), dict(loop=-1), dict(loop=70000), dict(encoder="pillow")):
        with pytest.raises(ValueError):
            GifWriter(io.BytesIO(), **dict(dict(width=w, height=h, fps=25), **kw))
    with pytest.raises(ValueError):
        write_gif("unused.gif", np.zeros((0, h, w), np.uint8), pal, 25, encoder="host")


def test_write_gif_on_the_host_encoder(tmp_path):
    from dither_pie_amd.gif import write_gif
    rs = np.random.RandomState(23)
    pal = _palette(rs, 16)
    planes = gr.content("tile", rs, 6, 20, 28, 16)
    path = tmp_path / "clip.gif"
    assert write_gif(str(path), planes, pal, 24, encoder="host") == 6
    im, got = _decode(path.read_bytes())
    assert im.n_frames == 6 and im.info["duration"] == 40 and all(np.array_equal(got[i], pal[planes[i]]) for i in range(6))


def test_process_video_gif_refuses_before_anything_starts(tmp_path):
    from dither_pie_amd.scenes import Scene
    from dither_pie_amd.video_processor import VideoProcessor
    pal = [(0, 0, 0), (255, 255, 255)]
    vp = VideoProcessor()
    vp.get_video_info = None                                            # anything past the argument checks would call it
    out = str(tmp_path / "o.gif")
    for bad in ([], [Scene(0, 9, pal), Scene(5, 12, pal)], [Scene(0, 9, None)], [Scene(0, 9, [(1, 2, 3)] * 257)]):
        with pytest.raises(ValueError):
            vp.process_video_gif("in.mp4", out, None, scene_palettes=bad)
    for kw in (dict(max_frames=0), dict(chunk_px=0), dict(chunk_px=-3)):
        with pytest.raises(ValueError):
            vp.process_video_gif("in.mp4", out, None, **kw)
    many = VideoProcessor(devices=[0, 1])
    many.get_video_info = None
    with pytest.raises(ValueError, match="one device"):
        many.process_video_gif("in.mp4", out, None)
    assert not os.path.exists(out)
