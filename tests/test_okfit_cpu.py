"""CPU tier of Oklab palette fitting (include/ditherpie_hip_okfit.h, backend.okfit, ColorReducer.generate_oklab_palette,
ClipPalette.oklab, ImageDitherer(palette_fit="oklab")): the agreement of the header, the ctypes table, the exported symbols and
the memory-discipline module (the rule tests/test_metric_cpu.py keeps for its header); the numpy statement tests/okfit_ref.py
against dp_okfit_host, through ctypes and through the stand-alone host_asan harness, on the cases of okfit_ref.cases() and on
what makes each of them a case; that the statement is a function of the colour multiset; the distortion conditions of four
synthetic images; the refusals of every entry point and of the Python layer, none of which needs a device."""
import ctypes as C
import inspect
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import metric_ref as mr
import okfit_ref as ok
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
FUNCTIONS = {"dp_okfit_hist_workspace_bytes", "dp_okfit_hist_count", "dp_okfit_hist_points", "dp_okfit_points_u32", "dp_okfit_workspace_bytes",
             "dp_okfit_fit", "dp_okfit_host"}
DEVICE_ENTRY_POINTS = {"dp_okfit_hist_count", "dp_okfit_hist_points", "dp_okfit_points_u32", "dp_okfit_fit"}
DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
CASES = ok.cases()


@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3])
            and a[0].dtype == b[0].dtype == np.uint8 and a[1].dtype == b[1].dtype == np.int32)


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_okfit.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_okfit_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == FUNCTIONS == set(_lib.EXPORTS_OKFIT)
    others = set()
    for name in dir(_lib):
        if name.startswith("EXPORTS") and name != "EXPORTS_OKFIT":
            others |= set(getattr(_lib, name))
    assert len(others) > 100 and not set(_lib.EXPORTS_OKFIT) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(_lib._SIGS_OKFIT[name][1]) == n_args, name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == DEVICE_ENTRY_POINTS
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version(lib):
    from dither_pie_amd import _lib, backend
    for name in _lib.EXPORTS_OKFIT:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: okfit.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_OKFIT:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    consts = {k: int(re.search(rf"#define\s+DP_OKFIT_{k}\s+(\d+)", _header_text()).group(1)) for k in ("MAX_COLORS", "MAX_ITER", "MAX_POINTS", "POINT_BYTES")}
    assert consts == dict(MAX_COLORS=256, MAX_ITER=10000, MAX_POINTS=1 << 24, POINT_BYTES=16)
    assert (backend.OKFIT_MAX_COLORS, backend.OKFIT_MAX_ITER, backend.OKFIT_MAX_POINTS, backend.OKFIT_POINT_BYTES) == (256, 10000, 1 << 24, 16)
    assert (ok.MAX_K, ok.MAX_ITER) == (256, 10000) and backend.OKFIT_POINT_DTYPE.itemsize == 16
    # workspace queries: pure host functions
    assert lib.dp_okfit_hist_workspace_bytes() >= 2 * 4096 * 4
    small, big = lib.dp_okfit_workspace_bytes(1, 1), lib.dp_okfit_workspace_bytes(1 << 24, 256)
    assert 0 < small < big and big - small >= 4 * ((1 << 24) - 64) and lib.dp_okfit_workspace_bytes(300, 1) == lib.dp_okfit_workspace_bytes(300, 256)
    for n, K in ((0, 4), (-1, 4), ((1 << 24) + 1, 4), (5, 0), (5, 257)):
        assert lib.dp_okfit_workspace_bytes(n, K) == 0, (n, K)


# ---------------------------------------------------------------------------------------------------- statement = host
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_statement_equals_the_numpy_statement(lib, name):
    from dither_pie_amd import backend
    codes, counts, K, max_iter = CASES[name]
    want = ok.fit_points(codes, counts, K, max_iter)
    got = backend.okfit_host(codes, counts, K, max_iter)
    assert same(got, want), (name, got, want)
    assert want[0].shape == (K, 3) and 1 <= want[2] <= max_iter
    have = {tuple(c) for c in ok.colours_of(codes).tolist()}
    assert all(tuple(c) in have for c in want[0].tolist())              # every entry is a colour of the input


def test_what_makes_each_case_a_case():
    fit = {name: ok.fit_points(*CASES[name]) for name in CASES}
    lab = lambda rgb: mr.lab(np.array(rgb, np.uint8)).astype(np.int64)   # noqa: E731
    d = lambda a, b: int(((lab(a) - lab(b)) ** 2).sum())                # noqa: E731
    # n < K: duplicates appear and are kept; n = K: every point is an entry, the distortion is 0
    pal = fit["n1_k3_duplicates"][0]
    assert pal.tolist() == [[12, 200, 77]] * 3 and fit["n1_k3_duplicates"][3] == 0
    pal = fit["n5_k16_duplicates"][0]
    assert len({tuple(c) for c in pal.tolist()}) == 5 and np.array_equal(pal[5:], np.repeat(pal[:1], 11, 0)) and fit["n5_k16_duplicates"][3] == 0
    pal = fit["n16_k16"][0]
    assert len({tuple(c) for c in pal.tolist()}) == 16 and fit["n16_k16"][3] == 0
    assert fit["n300_k1"][2] == 2                                       # K = 1: the mean, then "nothing changed"
    # one Lab, two colours: the lower code is centre 0 (equal counts), its twin has product 0; K = 3 has no third Lab
    a, b = ok.SAME_LAB
    assert a != b and np.array_equal(lab(a), lab(b)) and ok.code_of(a) < ok.code_of(b)
    assert fit["same_lab_code_order_decides"][0].tolist() == [list(a), [255, 255, 255]]
    assert fit["same_lab_k3_repeats_centre_0"][0].tolist() == [list(a), [255, 255, 255], list(a)]
    assert np.array_equal(fit["same_lab_k3_repeats_centre_0"][1][2], fit["same_lab_k3_repeats_centre_0"][1][0])
    # a point as far from centre 0 as from centre 1 goes to centre 0: centre 0 moved off A, centre 1 stayed on B
    p, A, B = ok.EQUIDISTANT
    assert d(p, A) == d(p, B) == 27996362 and lab(A).tolist() != lab(B).tolist()
    centres = fit["equidistant_centre_index_decides"][1].astype(np.int64)
    assert np.array_equal(centres[1], lab(B)) and not np.array_equal(centres[0], lab(A))
    assert np.array_equal(centres[0], (2 * (1000 * lab(A) + lab(p)) + 1001) // 2002)
    # a count of 2^32 - 2: the sums need 64 bits (count * L alone is above 2^45), the seeding product too
    codes, counts, K, _ = CASES["huge_count"]
    assert int(counts.max()) == (1 << 32) - 2 and int(counts.sum()) == (1 << 32) - 1
    heavy = lab((250, 120, 30))
    assert np.array_equal(fit["huge_count_k1"][1][0], (2 * (((1 << 32) - 2) * heavy + lab((1, 2, 3))) + (1 << 32) - 1) // (2 * ((1 << 32) - 1)))
    c = fit["huge_count_k1"][1][0].astype(np.int64)
    assert fit["huge_count_k1"][3] == ((1 << 32) - 2) * int(((heavy - c) ** 2).sum()) + int(((lab((1, 2, 3)) - c) ** 2).sum())
    # max_iter cuts the loop: one pass, two passes, and the full run needs more
    assert fit["max_iter_1"][2] == 1 and fit["max_iter_2"][2] == 2 and ok.fit_points(*CASES["max_iter_1"][:3])[2] > 2
    assert not np.array_equal(fit["max_iter_1"][1], fit["max_iter_2"][1])
    # negative a and b, every component's sum odd: half rounds up, towards zero for the negative ones
    la, lb = lab(ok.HALF_WAY[0]), lab(ok.HALF_WAY[1])
    assert ((la + lb) % 2).tolist() == [1, 1, 1] and la[1] < 0 and lb[1] < 0 and la[2] < 0 and lb[2] < 0
    assert fit["half_way_negative_mean"][1][0].tolist() == [8800, -659, -3351] == [(int(v) + 1) // 2 for v in la + lb]
    # the fixture: centre 2 has members in the first pass and none from the second on; it keeps its value and, without
    # members, takes its palette entry from all points
    codes, counts, K, _ = CASES["emptied_centre"]
    trace = ok.lloyd_trace(codes, counts, K)
    assert trace[0].min() >= 1 and trace[1:, 2].max() == 0 and len(trace) == fit["emptied_centre"][2] == 3
    pal, centres = fit["emptied_centre"][:2]
    P = mr.lab(ok.colours_of(codes)).astype(np.int64)
    assert pal[2].tolist() == ok.colours_of(codes)[int(np.argmin(((P - centres[2]) ** 2).sum(-1)))].tolist() == [94, 94, 94]
    assert ok.assign(P, centres.astype(np.int64))[0].tolist().count(2) == 0


def test_statement_is_a_function_of_the_colour_multiset():
    from dither_pie_amd import backend
    rs = np.random.RandomState(21)
    img = (rs.randint(0, 256, (40, 50, 3)) // 8 * 8).astype(np.uint8)    # 32^3 colours: many repeat
    want = ok.fit(img, 16)
    flat = img.reshape(-1, 3)
    assert same(ok.fit(flat[rs.permutation(len(flat))], 16), want)
    parts = np.split(flat[rs.permutation(len(flat))], [100, 777, 1500])  # the pixels split over several inputs: the counts add up
    codes = np.unique(np.concatenate([ok.points_of(p)[0] for p in parts]))
    counts = np.zeros(len(codes), np.int64)
    for p in parts:
        c, k = ok.points_of(p)
        counts[np.searchsorted(codes, c)] += k
    assert same(ok.fit_points(codes, counts, 16), want)
    assert same(backend.okfit_host(codes, counts, 16), want)
    assert same(ok.fit(img.transpose(1, 0, 2), 16), want)


# ---------------------------------------------------------------------------------------------------- distortion conditions
def synthetic_images():
    """Four 96 x 128 images: noise, a three-way gradient, a smooth "photo" with noise, dark-skewed noise."""
    h, w = 96, 128
    rs = np.random.RandomState(2024)
    y, x = np.mgrid[0:h, 0:w]
    noise = rs.randint(0, 256, (h, w, 3))
    gradient = np.stack([255 * x / (w - 1), 255 * y / (h - 1), 255 * (x + y) / (w + h - 2)], -1) + rs.randint(0, 4, (h, w, 3))
    photo = np.stack([128 + 100 * np.sin(x / 17.0) * np.cos(y / 23.0), 120 + 90 * np.sin((x + 2 * y) / 31.0), 100 + 80 * np.cos(x / 11.0 - y / 29.0)], -1) \
        + rs.normal(0, 6, (h, w, 3))
    dark = 255.0 * rs.rand(h, w, 3) ** 3
    return {name: np.clip(np.rint(v), 0, 255).astype(np.uint8) for name, v in (("noise", noise), ("gradient", gradient), ("photo", photo), ("dark", dark))}


def lab_distortion_of_palette(codes, counts, palette):
    P = mr.lab(ok.colours_of(codes)).astype(np.int64)
    return ok.distortion(P, counts, mr.lab(palette).astype(np.int64))


@pytest.mark.parametrize("name", ["noise", "gradient", "photo", "dark"])
def test_distortion_conditions_on_the_synthetic_images(lib, name):
    """Conditions on these inputs, not claims about images in general: the Lloyd passes end strictly below the seeding's
    distortion, and the palette's Oklab distortion is strictly below that of the same algorithm run on the RGB bytes.
    Ratios measured with these generators (fit / seeding, Oklab palette / RGB palette): DESIGN.md 4.3j."""
    from dither_pie_amd import backend
    img = synthetic_images()[name]
    codes, counts = ok.points_of(img)
    P = mr.lab(ok.colours_of(codes)).astype(np.int64)
    print(name, "distinct colours", len(codes))
    assert 8000 <= len(codes) <= 96 * 128
    for K in (4, 16, 64):
        pal, centres, n_iter, dist = backend.okfit_host(codes, counts, K)   # (equal to the numpy statement: the tests above)
        assert dist == ok.distortion(P, counts, centres.astype(np.int64))
        seeded = ok.distortion(P, counts, ok.seed(P, counts, K))
        rgb_pal = ok.fit_points(codes, counts, K, metric="rgb")[0]
        mine, theirs = lab_distortion_of_palette(codes, counts, pal), lab_distortion_of_palette(codes, counts, rgb_pal)
        print(f"{name} K={K}: n_iter {n_iter}, fit / seeding {dist / seeded:.4f}, oklab palette / rgb palette {mine / theirs:.4f}")
        assert dist < seeded, (name, K)
        assert mine < theirs, (name, K)


# ---------------------------------------------------------------------------------------------------- sanitizers
def test_host_statement_under_the_sanitizers(tmp_path):
    """The stand-alone harness (csrc/host_sanitize.cpp, built with -fsanitize=address,undefined; a program with its own main,
    nothing preloaded) runs okfit_check and okfit_host on arrays of exactly the stated size and prints what they give."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    names = sorted(CASES)
    bad = [  # (codes, counts, K, max_iter), the rule broken
        (([5, 5], [1, 1], 2, 10), 3), (([7, 5], [1, 1], 2, 10), 3), (([1 << 24], [1], 1, 10), 3), (([1, 2], [1, 0], 2, 10), 4),
        (([1, 2], [(1 << 32) - 1, 1], 2, 10), 4), (([1], [1], 0, 10), 1), (([1], [1], 257, 10), 2), (([1], [1], 2, 0), 1), (([1], [1], 2, 10001), 1),
        (([], [], 2, 10), 1),
    ]
    with open(tmp_path / "cases.bin", "wb") as f:
        for name in names:
            codes, counts, K, max_iter = CASES[name]
            f.write(np.array([len(codes), K, max_iter], "<i4").tobytes() + codes.astype("<u4").tobytes() + counts.astype("<u4").tobytes())
        for (codes, counts, K, max_iter), _ in bad:
            f.write(np.array([len(codes), K, max_iter], "<i4").tobytes() + np.array(codes, "<u4").tobytes() + np.array(counts, "<u4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    exe = os.path.join(CSRC, "build", "host_asan")
    r = subprocess.run([exe, "okfit", str(tmp_path / "cases.bin"), str(len(names) + len(bad))], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("okfit ")]
    assert len(lines) == len(names) + len(bad)
    for c, name in enumerate(names):
        codes, counts, K, max_iter = CASES[name]
        got = lines[c]
        assert got[:3] == ["okfit", str(c), "0"] and len(got) == 5 + 6 * K, (name, got[:5])
        res = (np.array(got[5:5 + 3 * K], np.int64).astype(np.uint8).reshape(K, 3), np.array(got[5 + 3 * K:], np.int64).astype(np.int32).reshape(K, 3),
               int(got[3]), int(got[4]))
        assert same(res, ok.fit_points(codes, counts, K, max_iter)), name
    for c, ((codes, counts, K, max_iter), rule) in enumerate(bad, len(names)):
        assert lines[c] == ["okfit", str(c), str(rule)], lines[c]        # a refused fit writes nothing
        if rule != 2:
            with pytest.raises(ValueError):
                ok.fit_points(np.array(codes, np.int64), np.array(counts, np.int64), K, max_iter)
    short = tmp_path / "short.bin"
    short.write_bytes(np.array([3, 2, 10, 1], "<i4").tobytes())
    assert subprocess.run([exe, "okfit", str(short), "1"], capture_output=True, env=env).returncode == 2


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
def _refused(lib, rc, want, fn):
    msg = lib.dp_last_error().decode()
    assert rc == want and fn in msg, (rc, msg)
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                 # (the product library spells out no status name)


def test_entry_point_refusals(lib):
    """Every refusal comes before any HIP call: the device addresses are made up and never dereferenced."""
    hist, pts, n_dev, ws = 0x10000000, 0x20000000, 0x30000008, 0x40000000
    need = lib.dp_okfit_hist_workspace_bytes()
    fn = "dp_okfit_hist_count"
    for kw in (dict(h=None), dict(h=hist + 8), dict(n=None), dict(n=n_dev + 4), dict(ws=None), dict(ws=ws + 8), dict(wsb=need - 1), dict(wsb=0)):
        v = dict(dict(h=hist, n=n_dev, ws=ws, wsb=need), **kw)
        _refused(lib, lib.dp_okfit_hist_count(v["h"], v["n"], v["ws"], v["wsb"], None), DP_EINVAL, fn)
    fn = "dp_okfit_hist_points"
    for kw in (dict(h=None), dict(h=hist + 4), dict(p=None), dict(p=pts + 8), dict(cap=-1), dict(cap=(1 << 24) + 1), dict(n=None), dict(n=n_dev + 2),
               dict(ws=None), dict(ws=ws + 4), dict(wsb=need - 1)):
        v = dict(dict(h=hist, p=pts, cap=100, n=n_dev, ws=ws, wsb=need), **kw)
        _refused(lib, lib.dp_okfit_hist_points(v["h"], v["p"], v["cap"], v["n"], v["ws"], v["wsb"], None), DP_EINVAL, fn)
    fn = "dp_okfit_points_u32"
    for kw in (dict(c=None), dict(k=None), dict(p=None), dict(c=0x1002), dict(k=0x2001), dict(p=pts + 8), dict(n=-1), dict(n=(1 << 24) + 1)):
        v = dict(dict(c=0x1000, k=0x2000, n=10, p=pts), **kw)
        _refused(lib, lib.dp_okfit_points_u32(v["c"], v["k"], v["n"], v["p"], None), DP_EINVAL, fn)
    assert lib.dp_okfit_points_u32(None, None, 0, None, None) == DP_OK   # nothing to do is not an error, and launches nothing
    fn = "dp_okfit_fit"
    n_iter = C.c_int(-7)
    need = lib.dp_okfit_workspace_bytes(300, 16)
    ok_args = dict(p=pts, n=300, K=16, it=100, pal=0x50000001, cen=0x60000004, dist=0x70000008, out=C.byref(n_iter), ws=ws, wsb=need)

    def fit(**kw):
        v = dict(ok_args, **kw)
        return lib.dp_okfit_fit(v["p"], v["n"], v["K"], v["it"], v["pal"], v["cen"], v["dist"], v["out"], v["ws"], v["wsb"], None)

    for kw in (dict(p=None), dict(p=pts + 8), dict(n=0), dict(n=-3), dict(n=(1 << 24) + 1), dict(K=0), dict(K=-1), dict(it=0), dict(it=10001), dict(it=-1),
               dict(pal=None), dict(cen=None), dict(cen=0x60000002), dict(dist=None), dict(dist=0x70000004), dict(out=None), dict(ws=None),
               dict(ws=ws + 8), dict(wsb=need - 1), dict(wsb=0), dict(K=0, n=0), dict(K=300, n=0), dict(K=300, it=0)):
        _refused(lib, fit(**kw), DP_EINVAL, fn)
    for K in (257, 1000):
        _refused(lib, fit(K=K), DP_EUNSUPPORTED, fn)
    assert n_iter.value == -7
    fn = "dp_okfit_host"
    codes, counts = np.array([1, 2, 3], np.uint32), np.array([1, 1, 1], np.uint32)
    pal, cen, dist = np.full((4, 3), 9, np.uint8), np.full((4, 3), 9, np.int32), C.c_uint64(5)
    host_ok = dict(c=codes.ctypes.data, k=counts.ctypes.data, n=3, K=4, it=10, pal=pal.ctypes.data, cen=cen.ctypes.data, out=C.byref(n_iter), d=C.byref(dist))

    def host(**kw):
        v = dict(host_ok, **kw)
        return lib.dp_okfit_host(v["c"], v["k"], v["n"], v["K"], v["it"], v["pal"], v["cen"], v["out"], v["d"])

    down, zero, big = np.array([1, 3, 3], np.uint32), np.array([1, 0, 1], np.uint32), np.array([(1 << 32) - 2, 1, 1], np.uint32)
    wide = np.array([1, 2, 1 << 24], np.uint32)
    for kw in (dict(c=None), dict(k=None), dict(pal=None), dict(cen=None), dict(out=None), dict(d=None), dict(n=0), dict(n=-1), dict(K=0), dict(it=0),
               dict(it=10001), dict(c=down.ctypes.data), dict(c=wide.ctypes.data), dict(k=zero.ctypes.data), dict(k=big.ctypes.data)):
        _refused(lib, host(**kw), DP_EINVAL, fn)
    _refused(lib, host(K=257), DP_EUNSUPPORTED, fn)
    assert (pal == 9).all() and (cen == 9).all() and dist.value == 5 and n_iter.value == -7
    assert host() == DP_OK and n_iter.value >= 1


def test_python_layer_refuses_before_the_device(monkeypatch):
    import torch
    from dither_pie_amd import backend, clip_palette, video_processor
    from dither_pie_amd import dithering_lib as d
    from PIL import Image

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(backend, "require_gpu", no_device)
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    pts = torch.zeros((4, 16), dtype=torch.uint8)
    for K, it, word in ((0, 100, "num_colors"), (-2, 100, "num_colors"), (257, 100, "256 colours"), (16, 0, "max_iter"), (16, 10001, "max_iter")):
        with pytest.raises(ValueError, match=word):
            backend.okfit(pts, K, it)
        with pytest.raises(ValueError, match=word):
            backend.okfit_host([1, 2], [1, 1], K, it)
        with pytest.raises(ValueError, match=word):
            d.ColorReducer.generate_oklab_palette(Image.new("RGB", (4, 4)), K, it)
        with pytest.raises(ValueError, match=word):
            d.ColorReducer.generate_oklab_palette_frames(pts, K, 1, it)
    with pytest.raises(TypeError, match="points"):
        backend.okfit(pts, 4)                                           # a CPU tensor is no point list
    for codes, counts, word in (([2, 1], [1, 1], "ascending"), ([1, 1 << 24], [1, 1], "ascending"), ([1, 2], [1, 0], "counts"),
                                ([1, 2], [(1 << 32) - 1, 1], "counts"), ([1, 2], [1], "same length"), ([], [], "same length")):
        with pytest.raises(ValueError, match=word):
            backend.okfit_host(codes, counts, 2)
        with pytest.raises(ValueError, match=word):
            backend.okfit_points(codes, counts)

    class Clip(clip_palette.ClipPalette):                               # the checks of oklab_fit, without the constructor's device
        def __init__(self, use_gamma, n):
            self.use_gamma, self._n = use_gamma, n
        n_pixels = property(lambda self: self._n)
    with pytest.raises(ValueError, match="no pixels"):
        Clip(False, 0).oklab(16)
    with pytest.raises(ValueError, match="256 colours"):
        Clip(False, 10).oklab(257)
    with pytest.raises(ValueError, match="256 colours"):
        Clip(False, 10).oklab_fit(300)
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        Clip(True, 10).oklab(16)
    with pytest.raises(ValueError, match="max_iter"):
        Clip(False, 10).oklab(16, max_iter=0)
    vp = video_processor.VideoProcessor()
    for call in (lambda **kw: vp.scan_palette("no_such_file.mp4", "oklab", **kw), lambda **kw: vp.scan_scenes("no_such_file.mp4", "oklab", **kw)):
        with pytest.raises(ValueError, match="256 colours"):
            call(num_colors=257)
        with pytest.raises(ValueError, match="use_gamma.*oklab"):
            call(num_colors=16, use_gamma=True)
    with pytest.raises(ValueError, match="'oklab'"):
        vp.scan_palette("no_such_file.mp4", "cielab", 16)
    with pytest.raises(ValueError, match="'oklab'"):
        vp.scan_scenes("no_such_file.mp4", "cielab", 16)


# ---------------------------------------------------------------------------------------------------- ImageDitherer(palette_fit=...)
def test_image_ditherer_palette_fit(monkeypatch):
    from dither_pie_amd import dithering_lib as d
    from PIL import Image
    params = list(inspect.signature(d.ImageDitherer.__init__).parameters)
    assert params[-2:] == ["palette_fit", "metric"] and inspect.signature(d.ImageDitherer.__init__).parameters["palette_fit"].default == "median_cut"
    assert d.PALETTE_FITS == ("median_cut", "oklab")
    rs = np.random.RandomState(4)
    img = rs.randint(0, 256, (12, 10, 3)).astype(np.uint8)
    want = d.ColorReducer.reduce_colors(Image.fromarray(img, "RGB"), 8)
    for kw in ({}, dict(palette_fit="median_cut"), dict(metric="oklab")):   # the default is today's median cut, whatever the metric
        x = d.ImageDitherer(num_colors=8, palette=None, **kw)
        assert x.palette_fit == "median_cut"
        x._ensure_palette(img)
        assert x.palette == want and len(want) == 8
    g = d.ImageDitherer(num_colors=8, palette=None, use_gamma=True)
    g._ensure_palette(img)
    from dither_pie_amd import _tables
    assert g.palette == d.ColorReducer.reduce_colors(Image.fromarray(_tables.LUT_IN[img], "RGB"), 8)
    old = d.ImageDitherer(palette=[(0, 0, 0)])
    del old.__dict__["palette_fit"]                                     # an object pickled before the attribute existed
    back = pickle.loads(pickle.dumps(old))
    assert "palette_fit" not in back.__dict__ and back.palette_fit == "median_cut" and back._check_palette_fit() == "median_cut"
    new = pickle.loads(pickle.dumps(d.ImageDitherer(palette=None, palette_fit="oklab", metric="rgb")))
    assert new.palette_fit == "oklab" and new.metric == "rgb"            # independent of the metric
    assert d.ImageDitherer(palette=None, palette_fit="oklab", metric="oklab").palette_fit == "oklab"
    with pytest.raises(ValueError, match="palette_fit"):
        d.ImageDitherer(palette_fit="kmeans")
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        d.ImageDitherer(palette_fit="oklab", use_gamma=True)
    new.use_gamma = True                                                # ... also when it is switched on later: before any device call
    monkeypatch.setattr(d.ColorReducer, "generate_oklab_palette", lambda *a, **k: pytest.fail("the fit was started"))
    with pytest.raises(ValueError, match="use_gamma.*oklab"):
        new._ensure_palette(img)
    given = d.ImageDitherer(palette=[(1, 2, 3)], palette_fit="oklab")    # a given palette is kept: nothing is fitted
    given._ensure_palette(img)
    assert given.palette == [(1, 2, 3)]
