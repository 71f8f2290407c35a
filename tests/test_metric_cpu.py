"""CPU tier of the Oklab colour metric (include/ditherpie_hip_metric.h, ImageDitherer(metric="oklab")): the agreement of the
header, the ctypes table, the exported symbols and the memory-discipline module (the rule tests/test_voidcluster_cpu.py keeps
for its header); the LIN literal, in Python and in C, against its formula and pin; the known answers and the all-colours pin
of (L, a, b) through dp_metric_lab_host; dp_metric_top2_host against the numpy statement tests/metric_ref.py; that the metric
is not RGB; the refusals of the host entry points; the Python surface; the host statements under the sanitizers as a
stand-alone program."""
import ctypes as C
import hashlib
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import metric_ref as mr
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
FUNCTIONS = {"dp_palette_create_metric", "dp_palette_metric", "dp_metric_prepare", "dp_metric_table_bytes", "dp_metric_ordered_u8",
             "dp_metric_lab_u8", "dp_metric_lab_host", "dp_metric_top2_host"}
KNOWN = {(0, 0, 0): (0, 0, 0), (255, 255, 255): (16383, 0, 0), (255, 0, 0): (10288, 3683, 2061), (0, 255, 0): (14195, -3833, 2940),
         (0, 0, 255): (7404, -532, -5104), (128, 128, 128): (9828, 0, 0), (1, 2, 3): (1339, -63, -118), (12, 200, 77): (11902, -2925, 1880)}
DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], axis=1).astype(np.uint8)        # the order r | g<<8 | b<<16


def palette(K, seed, duplicate=False):
    pal = np.random.RandomState(seed).randint(0, 256, (K, 3)).astype(np.float32)
    if duplicate:
        pal[K - 2] = pal[1]                                             # entry 1 twice: the lowest index wins, second is the duplicate
    return pal


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_metric.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_metric_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == FUNCTIONS == set(_lib.EXPORTS_METRIC)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
              | set(_lib.EXPORTS_PNG) | set(_lib.EXPORTS_PNG_DYN) | set(_lib.EXPORTS_PATTERN) | set(_lib.EXPORTS_PNG_FILE)
              | set(_lib.EXPORTS_DOTDIFF) | set(_lib.EXPORTS_CELLS) | set(_lib.EXPORTS_VOIDCLUSTER))
    assert not set(_lib.EXPORTS_METRIC) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_METRIC[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == {"dp_metric_ordered_u8", "dp_metric_lab_u8"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = (with_dev | {"dp_metric_prepare"}) - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version(lib):
    from dither_pie_amd import _lib, backend, dithering_lib
    for name in _lib.EXPORTS_METRIC:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: metric.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_METRIC:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    consts = {k: int(re.search(rf"#define\s+DP_METRIC_{k}\s+(\d+)", _header_text()).group(1)) for k in ("RGB", "OKLAB", "TABLE_BYTES")}
    assert (consts["RGB"], consts["OKLAB"]) == (_lib.METRIC_RGB, _lib.METRIC_OKLAB) == (0, 1) and consts["TABLE_BYTES"] == 2 << 24
    assert backend.METRICS == dithering_lib.METRICS == mr.METRICS == ("rgb", "oklab")
    assert lib.dp_palette_metric(None) == -1 and lib.dp_metric_table_bytes(None) == 0


# ---------------------------------------------------------------------------------------------------- the definition
def test_lin_literal_in_python_and_in_c():
    want = mr.lin_formula()
    assert np.array_equal(mr.LIN, want)
    assert hashlib.sha256(mr.LIN.astype("<u2").tobytes()).hexdigest()[:16] == "fdb7af3c01815a21"
    assert mr.LIN[[1, 10, 11, 12, 128, 254]].tolist() == [20, 199, 219, 241, 14146, 64952] and mr.LIN[0] == 0 and mr.LIN[255] == 65535
    u = np.arange(256) / 255.0                                          # no value near a rounding boundary: any libm gives the table
    exact = 65535.0 * np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)
    assert np.abs(exact - np.floor(exact) - 0.5).min() > 0.0015
    with open(os.path.join(CSRC, "host_logic.h")) as f:
        text = f.read()
    body = re.search(r"#define DP_METRIC_LIN_VALUES \\\n((?:.*\\\n)*.*)\n", text).group(1)
    c_lin = [int(v) for v in re.findall(r"\d+", body)]
    assert c_lin == want.tolist()
    for name, m in (("A", mr.A), ("B", mr.B)):                          # ... and the two matrices
        row = re.search(rf"kMetric{name}\[3\]\[3\] = (\{{\{{.*?\}}\}});", text).group(1)
        assert [int(v) for v in re.findall(r"-?\d+", row)] == m.reshape(-1).tolist(), name
    assert mr.A.sum(1).tolist() == [65536] * 3 and mr.B.sum(1).tolist() == [4096, 0, 0]


def test_cube_root_is_exact():
    c = mr.icbrt32(np.arange(65536))
    big = np.arange(65536, dtype=np.int64) << 32
    assert np.all(c ** 3 <= big) and np.all((c + 1) ** 3 > big) and c[0] == 0 and c[1] == 1625 and c[65535] == 65535


def test_known_answers(lib):
    from dither_pie_amd import backend
    rgb = np.array(list(KNOWN), np.uint8)
    want = np.array(list(KNOWN.values()), np.int32)
    assert np.array_equal(mr.lab(rgb), want)
    assert np.array_equal(backend.metric_lab_host(rgb), want)
    assert np.array_equal(mr.lab(rgb, "rgb"), rgb.astype(np.int32))


def test_all_colours_pin_range_and_grey_axis(lib):
    rgb = all_colours()
    got = np.full((1 << 24, 3), 12345, np.int32)
    assert lib.dp_metric_lab_host(rgb.ctypes.data, 1 << 24, got.ctypes.data) == DP_OK, lib.dp_last_error()
    assert hashlib.sha256(got.astype("<i4").tobytes()).hexdigest()[:16] == "fe5bcca474e0af41"
    assert got.min(0).tolist() == [0, -3833, -5104] and got.max(0).tolist() == [16383, 4526, 3253]
    grey = np.arange(256) * 0x010101
    assert not got[grey, 1:].any() and np.all(np.diff(got[grey, 0]) > 0)   # a = b = 0 exactly, L strictly increasing
    sample = np.random.RandomState(3).randint(0, 1 << 24, 1 << 16)
    assert np.array_equal(got[sample], mr.lab(rgb[sample]))             # ... and the statement agrees where it is sampled
    d_max = 408098306                                                    # the largest distance over the cube (black to white is less)
    far = ((got[0xFF0000].astype(np.int64) - got[0x00FF00]) ** 2).sum()
    assert far <= d_max < 2 ** 29


@pytest.mark.parametrize("K, dup", [(1, False), (2, False), (5, True), (16, False), (256, False)])
def test_top2_host_against_the_statement(lib, K, dup):
    from dither_pie_amd import backend
    rs = np.random.RandomState(100 + K)
    pal = palette(K, 200 + K, dup)
    rgb = rs.randint(0, 256, (1 << 16, 3)).astype(np.uint8)
    rgb[:K] = pal.astype(np.uint8)                                      # colours equal to palette entries
    w0, w1, d0, d1 = mr.top2(rgb, pal, want_d=True)
    g0, g1 = backend.metric_top2_host(rgb, pal)
    assert g0.dtype == np.uint8 and np.array_equal(g0, w0) and np.array_equal(g1, w1)
    assert np.all(d0[:K] == 0) and np.all(d0 <= d1)
    if K == 1:
        assert not g0.any() and not g1.any()
    if dup:
        assert g0[1] == 1 and g1[1] == K - 2 and g0[K - 2] == 1 and g1[K - 2] == K - 2     # the lowest index wins, second is the duplicate
        assert d0[1] + d1[1] == 0
        thr = np.zeros((1, 1), np.float32)                              # f = 0 when the sum is 0: nearest even at t = 0
        assert mr.ordered_indices(rgb[1:2].reshape(1, 1, 3), pal, thr)[0, 0] == 1
        assert np.array_equal(mr.ordered_indices(rgb.reshape(256, 256, 3), pal, thr).reshape(-1)[d0 > 0], w1[d0 > 0])
    r0, r1 = backend.metric_top2_host(rgb, pal, "rgb")                  # metric 0: the same pair order on the bytes
    x0, x1 = mr.top2(rgb, pal, "rgb")
    assert np.array_equal(r0, x0) and np.array_equal(r1, x1)


def test_the_metric_is_not_rgb(orc):
    """Guards against wiring the metric to the RGB path: on a seeded 16-colour palette the Oklab nearest differs from the
    oracle's RGB nearest on more than a tenth of 2^16 random colours (30.9 % over all 2^24 for RandomState(7))."""
    from dither_pie_amd import backend
    pal = np.random.RandomState(7).randint(0, 256, (16, 3)).astype(np.float32)
    rgb = np.random.RandomState(8).randint(0, 256, (256, 256, 3)).astype(np.uint8)
    rgb_idx = orc.ordered_u8(rgb, pal, pal.astype(np.uint8), None, "none", want_idx=True)[1]
    lab_idx = backend.metric_top2_host(rgb, pal)[0]
    share = float((lab_idx != rgb_idx).mean())
    print("nearest differs on", share)
    assert share > 0.1


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
def _refused(lib, rc, want, fn):
    msg = lib.dp_last_error().decode()
    assert rc == want and fn in msg, (rc, msg)
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                 # (the product library spells out no status name)


def test_host_entry_point_refusals(lib):
    rgb = np.zeros((4, 3), np.uint8)
    lab = np.full((4, 3), 77, np.int32)
    pal = palette(5, 1)
    i0, i1 = np.full(4, 9, np.uint8), np.full(4, 9, np.uint8)
    _refused(lib, lib.dp_metric_lab_host(None, 4, lab.ctypes.data), DP_EINVAL, "dp_metric_lab_host")
    _refused(lib, lib.dp_metric_lab_host(rgb.ctypes.data, 4, None), DP_EINVAL, "dp_metric_lab_host")
    _refused(lib, lib.dp_metric_lab_host(rgb.ctypes.data, -1, lab.ctypes.data), DP_EINVAL, "dp_metric_lab_host")
    assert lib.dp_metric_lab_host(None, 0, None) == DP_OK
    ok = dict(rgb=rgb.ctypes.data, n=4, pal=pal.ctypes.data, K=5, metric=1, i0=i0.ctypes.data, i1=i1.ctypes.data)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_metric_top2_host(v["rgb"], v["n"], v["pal"], v["K"], v["metric"], v["i0"], v["i1"])

    for bad in (dict(rgb=None), dict(pal=None), dict(i0=None), dict(i1=None), dict(n=-1), dict(K=0), dict(metric=2), dict(metric=-1)):
        _refused(lib, call(**bad), DP_EINVAL, "dp_metric_top2_host")
    big = palette(257, 2)
    frac = np.array([[0, 0, 0], [10.5, 3, 3]], np.float32)
    wide = np.array([[0, 0, 0], [256, 3, 3]], np.float32)
    low = np.array([[0, 0, 0], [-1, 3, 3]], np.float32)
    for p in (big, frac, wide, low):
        _refused(lib, call(pal=p.ctypes.data, K=len(p)), DP_EUNSUPPORTED, "dp_metric_top2_host")
    assert (i0 == 9).all() and (i1 == 9).all() and (lab == 77).all()
    # the palette constructor refuses before any HIP call: nothing was made
    handle = C.c_void_p(0x1234)
    outc = np.zeros((257, 3), np.uint8)
    for metric in (2, -1):
        _refused(lib, lib.dp_palette_create_metric(pal.ctypes.data, outc.ctypes.data, 5, metric, C.byref(handle)), DP_EINVAL, "dp_palette_create_metric")
    for p in (big, frac, wide, low):
        _refused(lib, lib.dp_palette_create_metric(p.ctypes.data, outc.ctypes.data, len(p), 1, C.byref(handle)), DP_EUNSUPPORTED,
                 "dp_palette_create_metric")
    for kw in (dict(p=None), dict(o=None), dict(K=0), dict(h=None)):
        v = dict(dict(p=pal.ctypes.data, o=outc.ctypes.data, K=5, h=C.byref(handle)), **kw)
        _refused(lib, lib.dp_palette_create_metric(v["p"], v["o"], v["K"], 1, v["h"]), DP_EINVAL, "dp_palette_create_metric")
    assert handle.value == 0x1234
    _refused(lib, lib.dp_metric_prepare(None), DP_EINVAL, "dp_metric_prepare")
    _refused(lib, lib.dp_metric_lab_u8(None, 0x1000, 4, None), DP_EINVAL, "dp_metric_lab_u8")
    _refused(lib, lib.dp_metric_lab_u8(0x1000, 0x1002, 4, None), DP_EINVAL, "dp_metric_lab_u8")        # lab_dev misaligned
    _refused(lib, lib.dp_metric_lab_u8(0x1000, 0x1000, -1, None), DP_EINVAL, "dp_metric_lab_u8")
    _refused(lib, lib.dp_metric_ordered_u8(0x1000, 0x2000, 1, 4, 4, 0, 0, None, 0, None, None), DP_EINVAL, "dp_metric_ordered_u8")


# ---------------------------------------------------------------------------------------------------- Python surface
def test_python_surface_errors_and_pickling(monkeypatch):
    from dither_pie_amd import backend
    from dither_pie_amd import dithering_lib as d
    import inspect
    assert list(inspect.signature(d.ImageDitherer.__init__).parameters)[-1] == "metric"
    assert inspect.signature(d.ImageDitherer.__init__).parameters["metric"].default == "rgb"
    assert list(inspect.signature(backend.Palette.__init__).parameters)[-1] == "metric"
    pal = [(0, 0, 0), (255, 255, 255), (200, 30, 30)]
    assert d.ImageDitherer(palette=pal).metric == "rgb"
    x = d.ImageDitherer(num_colors=3, dither_mode=d.DitherMode.BAYER, palette=pal, metric="oklab")
    back = pickle.loads(pickle.dumps(x))
    assert back.metric == "oklab" and back.palette == pal
    old = d.ImageDitherer(palette=pal)
    del old.__dict__["metric"]                                          # an object pickled before the attribute existed
    assert "metric" not in pickle.loads(pickle.dumps(old)).__dict__ and pickle.loads(pickle.dumps(old)).metric == "rgb"
    with pytest.raises(ValueError, match="metric"):
        d.ImageDitherer(palette=pal, metric="cielab")
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        d.ImageDitherer(palette=pal, use_gamma=True, metric="oklab")
    x.use_gamma = True                                                  # ... also when it is switched on later
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        x._check_metric(None)
    x.use_gamma = False

    # unsupported modes raise before any launch: no device is touched (a palette would need one)
    def no_device(*a, **k):
        raise AssertionError("a device palette was asked for")
    monkeypatch.setattr(d, "_device_palette", no_device)
    import torch
    frames = torch.zeros((4, 4, 3), dtype=torch.uint8)                  # a CPU tensor: .device is all the code may look at
    unsupported = [d.DitherMode.INTERLEAVED_GRADIENT_NOISE, d.DitherMode.ERROR_DIFFUSION, d.DitherMode.PERCEPTUAL, d.DitherMode.HYBRID,
                   d.DitherMode.ADAPTIVE_VARIANCE, d.DitherMode.OSTROMOUKHOV, d.DitherMode.RIEMERSMA, d.HalftoneDitherStrategy(),
                   d.WaveletDitherStrategy(), d.CellPaletteDitherStrategy()]
    for mode in unsupported:
        x = d.ImageDitherer(num_colors=3, dither_mode=mode, palette=pal, metric="oklab")
        name = mode.value if isinstance(mode, d.DitherMode) else type(mode).__name__
        with pytest.raises(ValueError, match=re.escape(name) + ".*oklab"):
            x.apply_dithering_frames(frames)
    for mode in (d.DitherMode.NONE, d.DitherMode.BAYER, d.DitherMode.BLUE_NOISE, d.DitherMode.POLKA_DOT, d.MatrixDitherStrategy(np.zeros((2, 2), np.float32)),
                 d.VoidAndClusterDitherStrategy(), d.PatternDitherStrategy(), d.DotDiffusionDitherStrategy()):
        x = d.ImageDitherer(num_colors=3, dither_mode=mode, palette=pal, metric="oklab")
        assert x._check_metric(x._get_dither_strategy(mode)) == "oklab"

    # backend: the argument errors that come before the device
    monkeypatch.setattr(backend, "require_gpu", no_device)
    with pytest.raises(ValueError, match="metric"):
        backend.Palette(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), metric="lab")
    with pytest.raises(ValueError, match="lut_in"):
        backend.Palette(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), np.arange(256, dtype=np.uint8), metric="oklab")
    with pytest.raises(ValueError, match="metric"):
        backend.metric_top2_host(np.zeros((1, 3), np.uint8), np.zeros((2, 3), np.float32), "lab")

    class FakePalette:                                                  # ordered() with IGN on a metric palette: ValueError, no launch
        metric, device, K, _h = "oklab", torch.device("cpu"), 2, None
    monkeypatch.setattr(backend, "_frames", lambda t: t.reshape(1, 4, 4, 3))
    monkeypatch.setattr(backend, "_check_out", lambda out, f: f)
    with pytest.raises(ValueError, match="gradient noise.*oklab"):
        backend.ordered(frames, FakePalette(), backend.MODE_IGN)


# ---------------------------------------------------------------------------------------------------- sanitizers
def test_host_statements_under_the_sanitizers(tmp_path):
    """The stand-alone harness (csrc/host_sanitize.cpp, built with -fsanitize=address,undefined; a program with its own main,
    nothing preloaded) runs metric_lab (with and without the cube-root table), metric_top2 and the ordered decision on buffers
    of exactly the stated size and prints what they give."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    rs = np.random.RandomState(11)
    cases = []
    for K, dup, n in ((1, False, 7), (2, False, 64), (5, True, 301), (16, False, 1000), (256, False, 513), (3, False, 0)):
        pal = palette(K, 300 + K, dup)
        rgb = rs.randint(0, 256, (n, 3)).astype(np.uint8)
        rgb[:min(n, K)] = pal.astype(np.uint8)[:min(n, K)]
        m = max(0, min(4, n - K))
        rgb[K:K + m] = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]], np.uint8)[:m]
        thr = rs.choice(np.array([0.0, 0.25, 0.5, 1.0, 0.49999997], np.float32), n).astype(np.float32)
        cases.append((pal, rgb, thr))
    with open(tmp_path / "cases.bin", "wb") as f:
        for pal, rgb, thr in cases:
            f.write(np.array([len(pal), len(rgb)], np.int32).tobytes() + pal.tobytes() + thr.tobytes() + rgb.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    exe = os.path.join(CSRC, "build", "host_asan")
    r = subprocess.run([exe, "metric", str(tmp_path / "cases.bin"), str(len(cases))], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    labs = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("lab ")]
    tops = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("top ")]
    assert len(labs) == len(tops) == len(cases)
    for c, (pal, rgb, thr) in enumerate(cases):
        n = len(rgb)
        assert int(labs[c][1]) == c and np.array_equal(np.array(labs[c][2:], np.int64).reshape(n, 3), mr.lab(rgb)), c
        got = np.array(tops[c][2:], np.int64).reshape(n, 3)
        w0, w1, d0, d1 = mr.top2(rgb, pal, want_d=True)
        s = (d0 + d1).astype(np.float64)
        f = np.where(s > 0, d0 / np.where(s > 0, s, 1.0), 0.0)
        assert int(tops[c][1]) == c and np.array_equal(got[:, 0], w0) and np.array_equal(got[:, 1], w1), c
        assert np.array_equal(got[:, 2], (f <= thr.astype(np.float64)).astype(np.int64)), c
    bad = tmp_path / "bad.bin"
    bad.write_bytes(np.array([257, 1], np.int32).tobytes())
    assert subprocess.run([exe, "metric", str(bad), "1"], capture_output=True, env=env).returncode == 2
