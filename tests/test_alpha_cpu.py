"""CPU tier of transparency (include/ditherpie_hip_alpha.h): the host entry points through ctypes against the numpy statements
(tests/alpha_ref.py), bit for bit; the coverage identity of the ordered mask for every alpha and matrix; the matte's end values; the
key in place; every refusal that happens before a HIP call, each naming its function; the agreement of the header, the ctypes table
and the exported symbols; the `alpha` mode of the stand-alone host_asan harness (nothing preloaded) against the statement; the tRNS
chunk of png.py decoded by Pillow, and files without the keyword byte for byte what they were; the ValueErrors of the Python layer."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_ref as ar
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
SHAPES = [(0, 4, 4), (3, 1, 1), (3, 3, 5), (3, 17, 19), (2, 33, 128)]
SETTINGS = ([dict(mode="threshold", threshold=t) for t in (0, 1, 128, 255, 256)]
            + [dict(mode="ordered", m=m, y0=y0, x0=x0) for m in (2, 4, 8) for y0, x0 in ((0, 0), (5, 3))])


def rgba_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    a = f[..., 3]
    for value, one_in in ((0, 4), (255, 4), (127, 8), (128, 8), (1, 16), (254, 16)):
        a[rng.integers(0, one_in, (n, h, w)) == 0] = value
    return f


def _backend_kw(kw):
    return {("matrix" if k == "m" else k): v for k, v in kw.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_entry_points_equal_the_statement(shape):
    from dither_pie_amd import backend
    n, h, w = shape
    src = rgba_frames(n, h, w, 31 * h + w)
    planes = np.random.default_rng(h).integers(0, 256, (n, h, w)).astype(np.uint8)
    for kw in SETTINGS:
        for matte in (None, (250, 10, 128), (0, 0, 0)):
            got, want = backend.alpha_split_host(src, matte=matte, **_backend_kw(kw)), ar.split(src, matte=matte, **kw)
            assert got[0].dtype == np.uint8 and got[1].dtype == np.uint8 and got[2].dtype == np.int64
            for g, x, what in zip(got, want, ("rgb", "mask", "masked")):
                assert np.array_equal(g, x), (what, kw, matte)
            assert set(np.unique(got[1]).tolist()) <= {0, 1}
            noisy = (got[1] * planes).astype(np.uint8)                   # any non-zero byte counts in key and join
            assert np.array_equal(backend.alpha_key_host(planes, noisy, 255), ar.key(planes, noisy, 255))
            assert np.array_equal(backend.alpha_join_host(got[0], noisy, (9, 8, 7)), ar.join(got[0], noisy, (9, 8, 7)))


def test_the_ordered_mask_covers_a_tile_as_stated():
    """Over a full m x m tile of constant alpha a exactly (2 m^2 a + 255) // 510 pixels are opaque; 0 is always transparent and 255
    never is; the count only grows with alpha.  On the statement and on the host entry point, at an origin that is no multiple of m."""
    from dither_pie_amd import backend
    for m in ar.MATRICES:
        before = 0
        for a in range(256):
            tile = np.full((1, m, m, 4), a, np.uint8)
            k = ar.mask_of(tile[..., 3], "ordered", m=m, y0=3, x0=5)
            opaque = int((k == 0).sum())
            assert opaque == ar.opaque_per_tile(a, m) == (2 * m * m * a + 255) // 510, (m, a)
            assert opaque >= before and (a != 0 or opaque == 0) and (a != 255 or opaque == m * m)
            before = opaque
            _, hk, masked = backend.alpha_split_host(tile, "ordered", matrix=m, y0=3, x0=5)
            assert np.array_equal(hk, k) and int(masked[0]) == m * m - opaque
    assert np.array_equal(ar.bayer_rank(2), [[0, 2], [3, 1]])


def test_matte_end_values():
    from dither_pie_amd import backend
    c = np.arange(256, dtype=np.uint8)
    for matte in ((0, 0, 0), (255, 255, 255), (13, 200, 77)):
        for a, want in ((255, np.stack([c, c, c], -1)), (0, np.broadcast_to(np.array(matte, np.uint8), (256, 3)))):
            src = np.concatenate([np.stack([c, c, c], -1), np.full((256, 1), a, np.uint8)], -1).reshape(1, 1, 256, 4)
            for impl in (ar.matte_of(src, matte), backend.alpha_split_host(src, matte=matte)[0]):
                assert np.array_equal(impl.reshape(256, 3), want), (matte, a)
    mid = ar.matte_of(np.array([[[[200, 100, 0, 128]]]], np.uint8), (0, 100, 255))
    assert mid.reshape(3).tolist() == [(200 * 128 + 127) // 255, 100, (255 * 127 + 127) // 255]


def test_key_in_place_through_the_descriptor():
    from dither_pie_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(2)
    planes = rng.integers(0, 200, (2, 5, 7)).astype(np.uint8)
    mask = rng.integers(0, 2, (2, 5, 7)).astype(np.uint8)
    want = ar.key(planes, mask, 200)
    a = _lib.AlphaKeyArgs(C.sizeof(_lib.AlphaKeyArgs), planes.ctypes.data, mask.ctypes.data, 2, 5, 7, 200, planes.ctypes.data, None)
    assert L.dp_alpha_key_host_u8(C.byref(a)) == DP_OK
    assert np.array_equal(planes, want)


# ---------------------------------------------------------------------------------------------------- refusals
def _fake_palette(k):
    """A stand-in palette handle whose K field (the first int) is k and whose host-side colour list is empty (tests/test_idiff_cpu.py)."""
    fake = C.create_string_buffer(8192)
    C.cast(fake, C.POINTER(C.c_int))[0] = k
    return fake


def test_every_refusal_names_its_function_and_happens_before_any_hip_call():
    """No device here: an entry point that reached a HIP call would answer DP_EHIP, not the code asked for."""
    from dither_pie_amd import _lib
    L = _lib.load()
    n, h, w = 2, 5, 7
    px = h * w
    rgba, rgb, mask = np.zeros((n, h, w, 4), np.uint8), np.full((n, h, w, 3), 9, np.uint8), np.full((n, h, w), 9, np.uint8)
    masked, planes, out = np.full(n + 1, -5, np.int64), np.zeros((n, h, w), np.uint8), np.full((n, h, w), 9, np.uint8)
    p = lambda a: a.ctypes.data                                           # noqa: E731
    split_ok = dict(struct_size=C.sizeof(_lib.AlphaSplitArgs), rgba_dev=p(rgba), n_frames=n, h=h, w=w, mode=1, threshold=128, m=4, y0=0, x0=0,
                    has_matte=0, rgb_dev=p(rgb), mask_dev=p(mask), masked_dev=p(masked), stream=None)
    key_ok = dict(struct_size=C.sizeof(_lib.AlphaKeyArgs), planes_dev=p(planes), mask_dev=p(mask), n_frames=n, h=h, w=w, key=7, out_dev=p(out), stream=None)
    join_ok = dict(struct_size=C.sizeof(_lib.AlphaJoinArgs), rgb_dev=p(rgb), mask_dev=p(mask), n_frames=n, h=h, w=w, rgba_dev=p(rgba), stream=None)
    common = [(dict(struct_size=0), DP_EINVAL), (dict(n_frames=-1), DP_EINVAL), (dict(h=0), DP_EINVAL), (dict(w=0), DP_EINVAL), (dict(h=-3), DP_EINVAL),
              (dict(h=1 << 16, w=1 << 15), DP_EINVAL), (dict(n_frames=65536), DP_EUNSUPPORTED)]
    table = [
        (("dp_alpha_split_u8", "dp_alpha_split_host_u8"), _lib.AlphaSplitArgs, split_ok, common + [
            (dict(struct_size=split_ok["struct_size"] + 8), DP_EINVAL), (dict(struct_size=split_ok["struct_size"] - 8), DP_EINVAL),
            (dict(rgba_dev=None), DP_EINVAL), (dict(rgb_dev=None), DP_EINVAL), (dict(mask_dev=None), DP_EINVAL), (dict(masked_dev=None), DP_EINVAL),
            (dict(mode=2), DP_EINVAL), (dict(mode=-1), DP_EINVAL), (dict(mode=0, threshold=-1), DP_EINVAL), (dict(mode=0, threshold=257), DP_EINVAL),
            (dict(m=3), DP_EINVAL), (dict(m=16), DP_EINVAL), (dict(m=0), DP_EINVAL), (dict(y0=-1), DP_EINVAL), (dict(x0=(1 << 30) + 1), DP_EINVAL),
            (dict(masked_dev=p(masked) + 4), DP_EINVAL), (dict(masked_dev=p(masked) + 1), DP_EINVAL),
            (dict(rgb_dev=p(rgba) + 5), DP_EINVAL), (dict(mask_dev=p(rgba) + 4 * n * px - 1), DP_EINVAL), (dict(mask_dev=p(rgb) + 3), DP_EINVAL),
            (dict(rgb_dev=p(mask)), DP_EINVAL)]),
        (("dp_alpha_key_u8", "dp_alpha_key_host_u8"), _lib.AlphaKeyArgs, key_ok, common + [
            (dict(struct_size=key_ok["struct_size"] + 8), DP_EINVAL), (dict(planes_dev=None), DP_EINVAL), (dict(mask_dev=None), DP_EINVAL),
            (dict(out_dev=None), DP_EINVAL), (dict(key=-1), DP_EINVAL), (dict(key=256), DP_EINVAL), (dict(out_dev=p(planes) + 1), DP_EINVAL),
            (dict(out_dev=p(mask)), DP_EINVAL), (dict(out_dev=p(mask) + n * px - 1), DP_EINVAL)]),
        (("dp_alpha_join_u8", "dp_alpha_join_host_u8"), _lib.AlphaJoinArgs, join_ok, common + [
            (dict(struct_size=join_ok["struct_size"] - 8), DP_EINVAL), (dict(rgb_dev=None), DP_EINVAL), (dict(mask_dev=None), DP_EINVAL),
            (dict(rgba_dev=None), DP_EINVAL), (dict(rgba_dev=p(rgb)), DP_EINVAL), (dict(rgba_dev=p(mask) - 4 * n * px + 1), DP_EINVAL)]),
    ]
    for names, cls, ok, refusals in table:
        for fn in names:
            f = getattr(L, fn)
            for kw, code in refusals:
                rc = f(C.byref(cls(**dict(ok, **kw))))
                msg = L.dp_last_error()
                assert rc == code and (fn + ":").encode() in msg, (fn, kw, rc, msg)
            assert f(None) == DP_EINVAL and (fn + ":").encode() in L.dp_last_error()
            assert f(C.byref(cls(**dict(ok, n_frames=0)))) == DP_OK     # n_frames = 0: DP_OK, nothing touched, the buffers may be NULL
            nulls = {k: None for k in ok if k.endswith("_dev")}
            assert f(C.byref(cls(**dict(ok, n_frames=0, **nulls)))) == DP_OK
    # the fields of the other mode are not looked at
    assert L.dp_alpha_split_host_u8(C.byref(_lib.AlphaSplitArgs(**dict(split_ok, mode=0, m=5, y0=-9)))) == DP_OK
    assert L.dp_alpha_split_host_u8(C.byref(_lib.AlphaSplitArgs(**dict(split_ok, mode=1, threshold=999)))) == DP_OK
    rgb[:], mask[:] = 9, 9
    assert (out == 9).all() and (masked[n:] == -5).all()


def test_the_masked_diffusions_refuse_before_any_hip_call():
    from dither_pie_amd import _lib
    L = _lib.load()
    keep, big = _fake_palette(16), _fake_palette(257)
    pal = C.cast(keep, C.c_void_p)
    n, h, w = 2, 5, 7
    px = h * w
    src, mask, out = np.zeros((n, h, w, 3), np.uint8), np.zeros((n, h, w), np.uint8), np.full((n, h, w, 3), 9, np.uint8)
    ws = np.zeros(4096, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    dx, dy, wt = np.array([1, -1, 0, 1], np.int32), np.array([0, 1, 1, 1], np.int32), np.array([7, 3, 5, 1], np.int32)
    classes = np.ascontiguousarray(ar.bayer_rank(4).astype(np.uint8))
    p = lambda a: a.ctypes.data                                           # noqa: E731
    id_ok = dict(struct_size=C.sizeof(_lib.AlphaIdiffArgs), in_dev=p(src), mask_dev=p(mask), out_dev=p(out), n_frames=n, h=h, w=w, pal=pal, dx=p(dx),
                 dy=p(dy), weight=p(wt), n_taps=4, divisor=16, strength256=256, workspace_dev=wsp, workspace_bytes=2048, stream=None)
    dot_ok = dict(struct_size=C.sizeof(_lib.AlphaDotdiffArgs), in_dev=p(src), mask_dev=p(mask), out_dev=p(out), n_frames=n, h=h, w=w, pal=pal,
                  classes_host=p(classes), m=4, strength256=256, stream=None)
    shared = [(dict(struct_size=0), DP_EINVAL), (dict(mask_dev=None), DP_EINVAL), (dict(in_dev=None), DP_EINVAL), (dict(out_dev=None), DP_EINVAL),
              (dict(pal=None), DP_EINVAL), (dict(n_frames=-1), DP_EINVAL), (dict(h=0), DP_EINVAL), (dict(w=0), DP_EINVAL),
              (dict(h=1 << 16, w=(1 << 14) + 1), DP_EINVAL), (dict(strength256=257), DP_EINVAL), (dict(out_dev=p(src)), DP_EINVAL),
              (dict(out_dev=p(src) + 3), DP_EINVAL), (dict(out_dev=p(mask)), DP_EINVAL), (dict(out_dev=p(mask) + n * px - 1), DP_EINVAL)]
    for fn, cls, ok, refusals in (
            ("dp_alpha_idiff_u8", _lib.AlphaIdiffArgs, id_ok, shared + [(dict(struct_size=id_ok["struct_size"] + 8), DP_EINVAL), (dict(dx=None), DP_EINVAL),
                                                                      (dict(n_taps=0), DP_EINVAL), (dict(n_taps=13), DP_EINVAL), (dict(divisor=0), DP_EINVAL),
                                                                      (dict(divisor=15), DP_EINVAL), (dict(workspace_dev=None), DP_EINVAL),
                                                                      (dict(workspace_dev=wsp + 8), DP_EINVAL), (dict(workspace_bytes=16), 5)]),
            ("dp_alpha_dotdiff_u8", _lib.AlphaDotdiffArgs, dot_ok, shared + [(dict(struct_size=dot_ok["struct_size"] - 8), DP_EINVAL),
                                                                          (dict(classes_host=None), DP_EINVAL), (dict(m=3), DP_EINVAL),
                                                                          (dict(classes_host=p(np.zeros(16, np.uint8))), DP_EINVAL)])):
        f = getattr(L, fn)
        for kw, code in refusals:
            rc = f(C.byref(cls(**dict(ok, **kw))))
            msg = L.dp_last_error()
            assert rc == code and (fn + ":").encode() in msg, (fn, kw, rc, msg)
        assert f(None) == DP_EINVAL and (fn + ":").encode() in L.dp_last_error()
        assert f(C.byref(cls(**dict(ok, n_frames=0)))) == DP_OK
        assert f(C.byref(cls(**dict(ok, n_frames=0, in_dev=None, mask_dev=None, out_dev=None, **({"workspace_dev": None} if "workspace_dev" in ok else {}))))) == DP_OK
        rc = f(C.byref(cls(**dict(ok, pal=C.cast(big, C.c_void_p)))))   # more than 256 colours
        assert rc == DP_EUNSUPPORTED and (fn + ":").encode() in L.dp_last_error() and b"256" in L.dp_last_error()
    assert (out == 9).all()


# ---------------------------------------------------------------------------------------------------- header, binding
STRUCTS = {"dp_alpha_split_args": "AlphaSplitArgs", "dp_alpha_key_args": "AlphaKeyArgs", "dp_alpha_join_args": "AlphaJoinArgs",
           "dp_alpha_idiff_args": "AlphaIdiffArgs", "dp_alpha_dotdiff_args": "AlphaDotdiffArgs"}


def test_header_and_binding_agree():
    from dither_pie_amd import _lib, backend
    with open(os.path.join(ROOT, "include", "ditherpie_hip_alpha.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}
    assert set(found) == set(_lib.EXPORTS_ALPHA) == {"dp_alpha_split_u8", "dp_alpha_split_host_u8", "dp_alpha_key_u8", "dp_alpha_key_host_u8",
                                                     "dp_alpha_join_u8", "dp_alpha_join_host_u8", "dp_alpha_idiff_u8", "dp_alpha_dotdiff_u8"}
    others = set()
    for name in dir(_lib):
        if name.startswith("EXPORTS") and name != "EXPORTS_ALPHA":
            others |= set(getattr(_lib, name))
    assert len(others) > 100 and not set(_lib.EXPORTS_ALPHA) & others
    for name, args in found.items():                                    # one descriptor each, and no stream PARAMETER anywhere
        assert len(_lib._SIGS_ALPHA[name][1]) == len([a for a in args.split(",") if a.strip()]) == 1, name
        assert not re.search(r"void\s*\*\s*stream\b", args)
    for cname, pyname in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (cname, cname), text, flags=re.S).group(1)
        fields = [re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        cls = getattr(_lib, pyname)
        assert fields == [n for n, _ in cls._fields_], cname
        assert fields[0] == "struct_size" and fields[-1] == "stream" and cls.struct_size.offset == 0 and C.sizeof(cls) % 8 == 0
    assert (C.sizeof(_lib.AlphaSplitArgs), C.sizeof(_lib.AlphaKeyArgs), C.sizeof(_lib.AlphaJoinArgs)) == (96, 64, 64)
    assert (C.sizeof(_lib.AlphaIdiffArgs), C.sizeof(_lib.AlphaDotdiffArgs)) == (120, 88)
    assert int(re.search(r"#define\s+DP_ALPHA_MAX_FRAMES\s+(\d+)", text).group(1)) == _lib.ALPHA_MAX_FRAMES == backend.ALPHA_MAX_FRAMES == 65535
    assert int(re.search(r"#define\s+DP_ALPHA_MAX_ORIGIN\s+(\d+)", text).group(1)) == _lib.ALPHA_MAX_ORIGIN == 1 << 30
    assert [int(re.search(r"#define\s+DP_ALPHA_%s\s+(\d+)" % n.upper(), text).group(1)) for n in _lib.ALPHA_MODES] == [0, 1]
    assert backend.ALPHA_MODES == ar.MODES and backend.ALPHA_MATRICES == ar.MATRICES


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_ALPHA:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert re.search(r"^SRCS = .*\balpha\.hip\b", f.read(), flags=re.M)


# ---------------------------------------------------------------------------------------------------- host logic under ASan / UBSan
@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([os.path.join(CSRC, "build", "host_asan")] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        return r.stdout.strip().split("\n")
    return run


def test_host_statements_under_the_sanitizers_equal_the_statement(harness, tmp_path):
    """Every setting through `host_asan alpha` on vectors of exactly the stated sizes: split, then key and join with the mask it made."""
    todo = []
    for i, (n, h, w) in enumerate(s for s in SHAPES if s[0]):
        for j, kw in enumerate(SETTINGS):
            todo.append((n, h, w, kw, j % 2 == 1, rgba_frames(n, h, w, 500 + 20 * i + j)))
    bad = [(1, 0, 4, 0, 128, 4, 0, 0), (1, 4, 4, 2, 128, 4, 0, 0), (1, 4, 4, 0, 257, 4, 0, 0), (1, 4, 4, 1, 0, 3, 0, 0), (1, 4, 4, 1, 0, 4, -1, 0),
           (65536, 4, 4, 0, 1, 4, 0, 0)]                                # rules 2, 4, 5, 6, 7, 3
    matte, fill, key = (250, 10, 128), (9, 8, 7), 201
    with open(tmp_path / "cases.bin", "wb") as f:
        for n, h, w, kw, has_matte, src in todo:
            md = ar.MODES.index(kw["mode"])
            f.write(np.array([n, h, w, md, kw.get("threshold", 0), kw.get("m", 0), kw.get("y0", 0), kw.get("x0", 0), int(has_matte), key], "<i4").tobytes())
            f.write(bytes(matte) + bytes(fill) + src.tobytes())
        for n, h, w, md, thr, m, y0, x0 in bad:
            f.write(np.array([n, h, w, md, thr, m, y0, x0, 0, key], "<i4").tobytes() + bytes(6))
    lines = harness("alpha", tmp_path / "cases.bin", len(todo) + len(bad), tmp_path / "out.bin")
    assert len(lines) == len(todo) + len(bad)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    at = 0
    for i, ((n, h, w, kw, has_matte, src), line) in enumerate(zip(todo, lines)):
        rgb, mask, masked = ar.split(src, matte=matte if has_matte else None, **kw)
        assert line.split() == ["alpha", str(i), "0", str(int(masked.sum()))], (line, kw)
        px = n * h * w
        parts = []
        for size in (3 * px, px, 8 * n, px, 4 * px):
            parts.append(raw[at:at + size])
            at += size
        assert np.array_equal(parts[0].reshape(rgb.shape), rgb) and np.array_equal(parts[1].reshape(mask.shape), mask), kw
        assert np.array_equal(parts[2].view(np.int64), masked)
        planes = (src[..., 0] % 200).astype(np.uint8)                   # (the harness keys the red channel mod 200)
        assert np.array_equal(parts[3].reshape(mask.shape), ar.key(planes, mask, key)), kw
        assert np.array_equal(parts[4].reshape(n, h, w, 4), ar.join(rgb, mask, fill)), kw
    assert at == len(raw)
    assert [ln.split()[2] for ln in lines[len(todo):]] == ["2", "4", "5", "6", "7", "3"]


# ---------------------------------------------------------------------------------------------------- png.py: tRNS
def test_a_transparent_container_decodes_in_pillow_and_files_without_the_keyword_are_unchanged():
    from PIL import Image
    from dither_pie_amd import backend, png
    rng = np.random.default_rng(8)
    for K, T in ((2, 1), (5, 0), (16, 15), (17, 3), (256, 255), (256, 0)):
        palette = rng.integers(0, 256, (K, 3)).astype(np.uint8)
        plane = rng.integers(0, K, (11, 13)).astype(np.uint8)
        plane[0, :3] = T
        depth = backend.png_depth(K)
        stream = backend.png_deflate_host(plane[None], depth)[0]
        plain = png.container(13, 11, depth, palette, stream)
        data = png.container(13, 11, depth, palette, stream, transparent=T)
        at = data.index(b"tRNS")
        assert data[at - 4:at] == (T + 1).to_bytes(4, "big") and data[at + 4:at + 5 + T] == b"\xff" * T + b"\x00"
        assert data.index(b"PLTE") < at < data.index(b"IDAT") and len(data) == len(plain) + 12 + T + 1 and b"tRNS" not in plain
        im = Image.open(io.BytesIO(data))
        assert im.mode == "P" and im.info["transparency"] == T
        rgba = np.asarray(im.convert("RGBA"))
        assert np.array_equal(rgba[..., :3], palette[plane]) and np.array_equal(rgba[..., 3] == 0, plane == T)
        assert set(np.unique(rgba[..., 3]).tolist()) <= {0, 255}
        for blocks in backend.PNG_BLOCKS:
            assert png.encode_png(plane, palette, encoder="host", blocks=blocks, transparent=T)[0] == png.container(
                13, 11, depth, palette, backend.png_deflate_host(plane[None], depth, None, blocks)[0], transparent=T)
        # without the keyword: byte-identical to the container as it always was
        assert png.encode_png(plane, palette, encoder="host")[0] == plain == png.encode_png(plane, palette, encoder="host", transparent=None)[0]
        for bad in (K, -1, 1.0, True, "0"):
            with pytest.raises(ValueError):
                png.container(13, 11, depth, palette, stream, transparent=bad)
            with pytest.raises(ValueError):
                png.encode_png(plane, palette, encoder="host", transparent=bad)
    with pytest.raises(TypeError):                                      # keyword only
        png.container(13, 11, 8, palette, stream, png.IDAT_BYTES, 3)
    import inspect
    for fn in (png.container, png.encode_png, png.write_png, png.write_png_sequence):
        prm = inspect.signature(fn).parameters["transparent"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is None


def test_write_png_takes_the_keyword(tmp_path):
    from PIL import Image
    from dither_pie_amd import png
    palette = [(0, 0, 0), (255, 0, 0), (0, 255, 0)]
    planes = np.array([[[0, 1], [2, 2]], [[2, 1], [0, 0]]], np.uint8)
    png.write_png(tmp_path / "a.png", planes[0], palette, encoder="host", transparent=2)
    assert Image.open(tmp_path / "a.png").info["transparency"] == 2
    paths = png.write_png_sequence(str(tmp_path / "f_%02d.png"), planes, palette, encoder="host", transparent=0)
    assert [Image.open(q).info["transparency"] for q in paths] == [0, 0]


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_alpha_mode_and_the_value_errors_of_the_python_layer():
    import inspect
    import pickle
    from dither_pie_amd import backend, dithering_lib as dl
    am = dl.AlphaMode()
    assert (am.mode, am.threshold, am.matrix, am.matte, am.fill) == ("threshold", 128, "4x4", None, (0, 0, 0))
    assert am._settings() == ("threshold", 128, 4, None, (0, 0, 0))
    assert pickle.loads(pickle.dumps(dl.AlphaMode("ordered", matrix="8x8", matte=(1, 2, 3))))._settings() == ("ordered", 128, 8, (1, 2, 3), (0, 0, 0))
    for kw in (dict(mode="soft"), dict(threshold=-1), dict(threshold=257), dict(threshold=1.5), dict(matrix="3x3"), dict(matrix=4), dict(matte=(1, 2)),
               dict(matte=(1, 2, 256)), dict(fill=None), dict(fill=(0.5, 0, 0)), dict(fill="red")):
        with pytest.raises(ValueError):
            dl.AlphaMode(**kw)._settings()
    # the constructor and the existing methods are what they were; alpha is asked for per call
    assert "alpha" not in inspect.signature(dl.ImageDitherer.__init__).parameters
    assert inspect.signature(dl.ImageDitherer.apply_dithering_png).parameters["alpha"].kind is inspect.Parameter.KEYWORD_ONLY
    # unsupported strategies: ValueError naming the supported ones, before anything touches a device (there is none here)
    for mode in (dl.DitherMode.ERROR_DIFFUSION, dl.DitherMode.RIEMERSMA, dl.DitherMode.OSTROMOUKHOV, dl.DitherMode.HYBRID, dl.HalftoneDitherStrategy(),
                 dl.CellPaletteDitherStrategy()):
        d = dl.ImageDitherer(num_colors=4, dither_mode=mode, palette=[(0, 0, 0), (255, 255, 255)])
        for call in (lambda: d.apply_dithering_frames_alpha(None, dl.AlphaMode()), lambda: d.apply_dithering_frames_indexed_alpha(None, dl.AlphaMode())):
            with pytest.raises(ValueError, match="IntegerErrorDiffusionDitherStrategy"):
                call()
    for mode in (dl.DitherMode.NONE, dl.DitherMode.BAYER, dl.DitherMode.BLUE_NOISE, dl.DitherMode.POLKA_DOT, dl.DitherMode.INTERLEAVED_GRADIENT_NOISE,
                 dl.PatternDitherStrategy(), dl.IntegerErrorDiffusionDitherStrategy(), dl.DotDiffusionDitherStrategy()):
        dl.ImageDitherer(num_colors=4, dither_mode=mode, palette=[(0, 0, 0)])._alpha_strategy()
    # K = 256: the key needs an entry of its own
    d = dl.ImageDitherer(dither_mode=dl.DitherMode.NONE, palette=[(i, i, i) for i in range(256)])
    with pytest.raises(ValueError, match="255"):
        d.apply_dithering_frames_indexed_alpha(None, dl.AlphaMode())
    with pytest.raises(ValueError, match="255"):
        dl.ImageDitherer(num_colors=256, dither_mode=dl.DitherMode.NONE).apply_dithering_frames_indexed_alpha(None, dl.AlphaMode())
    with pytest.raises(ValueError, match="AlphaMode"):
        dl.ImageDitherer(dither_mode=dl.DitherMode.NONE, palette=[(0, 0, 0)]).apply_dithering_frames_alpha(None, "threshold")
    # the wrappers refuse before the library
    src = np.zeros((1, 2, 2, 4), np.uint8)
    for kw in (dict(mode="x"), dict(threshold=300), dict(matrix=3), dict(matte=(1, 2)), dict(y0=-1), dict(x0=1.5)):
        with pytest.raises(ValueError):
            backend.alpha_split_host(src, **kw)
    for key in (-1, 256, 1.0):
        with pytest.raises(ValueError):
            backend.alpha_key_host(src[..., 0], src[..., 0], key)
    with pytest.raises(ValueError):
        backend.alpha_join_host(src[..., :3], src[..., 0], fill=(1, 2))
