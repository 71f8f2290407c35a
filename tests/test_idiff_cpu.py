"""CPU tier of integer error diffusion (include/ditherpie_hip_idiff.h, dithering_lib.IntegerErrorDiffusionDitherStrategy): the
agreement of the header, the ctypes table, the exported symbols and the memory-discipline module (the rule
tests/test_dotdiff_cpu.py keeps for its header); idiff_plan (host_logic.h) through the stand-alone host_asan harness against
the definition, for the reference's eight tap sets and for broken ones, on tap arrays of exactly the stated size; the refusals
of dp_idiff_u8 that happen before any HIP call; properties of the numpy statement (tests/idiff_ref.py) that follow from the
definition alone; the Python surface with no device."""
import ctypes as C
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import idiff_ref as ir
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_idiff.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_idiff_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_idiff_workspace_bytes", "dp_idiff_u8"} == set(_lib.EXPORTS_IDIFF)
    others = set()
    for name in dir(_lib):
        if name.startswith("EXPORTS") and name != "EXPORTS_IDIFF":
            others |= set(getattr(_lib, name))
    assert len(others) > 100 and not set(_lib.EXPORTS_IDIFF) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_IDIFF[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == {"dp_idiff_u8"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib, backend
    L = _lib.load()
    for name in _lib.EXPORTS_IDIFF:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: idiff.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_IDIFF:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    assert int(re.search(r"#define\s+DP_IDIFF_MAX_TAPS\s+(\d+)", _header_text()).group(1)) == backend.IDIFF_MAX_TAPS == ir.MAX_TAPS == 12
    assert L.dp_idiff_workspace_bytes(2, 130, 70) == 2 * 32 * 70         # O(w) per frame, whatever h is
    assert L.dp_idiff_workspace_bytes(2, 1, 70) == L.dp_idiff_workspace_bytes(2, 32768, 70)
    assert L.dp_idiff_workspace_bytes(-1, 4, 4) == L.dp_idiff_workspace_bytes(1, 0, 4) == L.dp_idiff_workspace_bytes(1, 4, 0) == 0
    with open(os.path.join(ROOT, "include", "ditherpie_hip_metric.h")) as f:
        assert "dp_idiff_u8" in f.read()                                # the list of entry points that use the metric names it


def test_reference_tap_sets_are_the_strategys():
    from dither_pie_amd.dithering_lib import ErrorDiffusionKernel as K
    assert sorted(ir.KERNELS) == sorted(K.list_kernels()) and len(ir.KERNELS) == 8
    for name, (taps, divisor) in ir.KERNELS.items():
        k = K.get_kernel(name)
        assert [tuple(t) for t in k["weights"]] == taps and k["divisor"] == divisor, name
        ir.check_taps(taps, divisor, 256)                               # every one satisfies the header's rules


# ---------------------------------------------------------------------------------------------------- idiff_plan under ASan / UBSan
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


def _record(taps, divisor, s256, n_taps=None):
    n = len(taps) if n_taps is None else n_taps
    return (np.array([n, divisor, s256], "<i4").tobytes()
            + b"".join(np.array([t[i] for t in taps[:max(n, 0)]], "<i4").tobytes() for i in range(3)))


EXPECTED_SKEW = {"floyd_steinberg": 2, "sierra_lite": 2, "atkinson": 2, "jjn": 3, "stucki": 3, "burkes": 3, "sierra": 3, "sierra_two_row": 3}


def test_plan_equals_the_definition_for_the_eight_tap_sets(harness, tmp_path):
    cases = [(name, s) for name in sorted(ir.KERNELS) for s in (0, 1, 77, 255, 256)]
    with open(tmp_path / "cases.bin", "wb") as f:
        for name, s in cases:
            f.write(_record(*ir.KERNELS[name], s))
    lines = harness("idiffplan", tmp_path / "cases.bin", len(cases))
    assert len(lines) == len(cases)
    for i, ((name, s), line) in enumerate(zip(cases, lines)):
        taps, divisor = ir.KERNELS[name]
        got = line.split()
        assert got[:3] == ["idiff", str(i), "0"], line
        q = [int(v) for v in got[5:]]
        assert int(got[3]) == len(taps) == len(q)
        assert q == ir.shares(taps, divisor, s) == [wt * s * 256 // divisor for _, _, wt in taps], (name, s)
        assert sum(q) <= 65536 and (s < 256 or sum(q) > 65536 - len(taps) or name == "atkinson")
        assert int(got[4]) == ir.skew(taps) == EXPECTED_SKEW[name], name
        for dx, dy, _ in taps:                                          # what the skew is for, and what the 8-column ring holds
            assert 1 <= int(got[4]) * dy + dx <= 8


def test_tap_cases_cover_the_skews_the_counts_and_the_spare_slots():
    """What tests/test_gpu_idiff.py runs beyond the eight variants: every case obeys the header; skews 1, 2 and 3 occur at
    least four times each, every tap count 1 .. 12 occurs, and each of the kernel's three instances (4, 7 and 12 tap slots)
    occurs with at least one spare slot."""
    cases = ir.tap_cases()
    assert cases == ir.tap_cases() and len(cases) >= 16 + ir.N_RANDOM_CASES          # a fixed list
    named = [sorted(taps) for taps, _ in ir.KERNELS.values()]
    for taps, divisor, s in cases:
        assert ir.check_taps(taps, divisor, s) == taps
        assert all(isinstance(v, int) for t in taps for v in t) and isinstance(divisor, int)
        assert sorted(taps) not in named or s != 256                  # none repeats a variant
    skews = [ir.skew(taps) for taps, _, _ in cases]
    counts = [len(taps) for taps, _, _ in cases]
    print("skews", [skews.count(v) for v in (1, 2, 3)], "tap counts", sorted(counts))
    assert set(skews) == {1, 2, 3} and min(skews.count(v) for v in (1, 2, 3)) >= 4
    assert set(counts) == set(range(1, ir.MAX_TAPS + 1))
    assert any(n < 4 for n in counts) and any(5 <= n < 7 for n in counts) and any(8 <= n < 12 for n in counts)
    for must in ([(1, 0, 1)], [(2, 0, 1)], [(0, 1, 1)], [(0, 2, 1)], [(-1, 2, 1)], [(-2, 2, 1)], [(-2, 1, 1)]):
        assert (must, 1, 256) in cases
    assert ([(-2, 1, 1), (2, 2, 1)], 2, 256) in cases and ([(2, 1, 1), (2, 2, 1)], 2, 256) in cases
    assert ([(1, 0, 7), (0, 1, 5), (1, 1, 3), (0, 2, 1)], 16, 256) in cases
    assert any(len(taps) == 2 and max(ir.skew(taps) * dy + dx for dx, dy, _ in taps) == 8 for taps, _, _ in cases)   # the ring depth
    assert any((-2, 1, 0) in taps for taps, _, _ in cases)
    assert any(sum(t[2] for t in taps) == 3 and divisor == 1000 for taps, divisor, _ in cases)
    assert any(s == 255 for _, _, s in cases)
    assert any(all(dy != 1 for _, dy, _ in taps) for taps, _, _ in cases) and any((1, 0) not in [t[:2] for t in taps] for taps, _, _ in cases)


def test_plan_equals_the_definition_for_the_tap_cases(harness, tmp_path):
    cases = ir.tap_cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        for taps, divisor, s in cases:
            f.write(_record(taps, divisor, s))
    lines = harness("idiffplan", tmp_path / "cases.bin", len(cases))
    assert len(lines) == len(cases)
    for i, ((taps, divisor, s), line) in enumerate(zip(cases, lines)):
        got = line.split()
        assert got[:3] == ["idiff", str(i), "0"], (line, taps)
        q = [int(v) for v in got[5:]]
        assert int(got[3]) == len(taps) == len(q), (line, taps)
        assert q == ir.shares(taps, divisor, s) and sum(q) <= 65536, (taps, divisor, s)
        assert int(got[4]) == ir.skew(taps), (line, taps)
        for dx, dy, _ in taps:
            assert dy == 0 or 1 <= int(got[4]) * dy + dx <= 8, (line, taps)


def test_plan_refuses_what_the_header_refuses(harness, tmp_path):
    fs, d = ir.KERNELS["floyd_steinberg"]
    jjn = ir.KERNELS["jjn"][0]
    big = 2 ** 31 - 1
    cases = [                                                           # (taps, divisor, strength256, n_taps given), the rule broken
        ((fs, d, 256, 0), 2), ((fs, d, 256, -1), 2), ((jjn + [(1, 1, 0)], 48, 256, None), 2),
        ((fs, 0, 256, None), 3), ((fs, -16, 256, None), 3), ((fs, d, -1, None), 4), ((fs, d, 257, None), 4),
        (([(0, 0, 1)], 1, 256, None), 5), (([(-1, 0, 1)], 1, 256, None), 5), (([(0, 3, 1)], 1, 256, None), 5), (([(3, 1, 1)], 1, 256, None), 5),
        (([(-3, 1, 1)], 1, 256, None), 5), (([(1, -1, 1)], 1, 256, None), 5), (([(1, 0, 1), (1, 0, 1)], 4, 256, None), 6),
        (([(1, 0, -1)], 4, 256, None), 7), ((fs, 15, 256, None), 8), (([(1, 0, big), (0, 1, big)], big, 256, None), 8),
        # accepted: the extremes of every rule
        (([(1, 0, big)], big, 256, None), 0), (([(1, 0, 0)], 1, 0, None), 0), ((jjn, 48, 256, None), 0), (([(-2, 1, 1), (2, 2, 1)], 2, 256, None), 0),
    ]
    with open(tmp_path / "cases.bin", "wb") as f:
        for (taps, divisor, s, n), _ in cases:
            f.write(_record(taps, divisor, s, n))
    lines = harness("idiffplan", tmp_path / "cases.bin", len(cases))
    for i, (((taps, divisor, s, n), rule), line) in enumerate(zip(cases, lines)):
        got = line.split()
        assert got[:3] == ["idiff", str(i), str(rule)], (line, taps)
        if rule:
            assert got[3:] == ["0", "0"], line                          # a refused plan is empty
            with pytest.raises(ValueError):
                ir.check_taps(taps if n is None else taps[:max(n, 0)], divisor, s)
    assert lines[-4].split()[5:] == ["65536"] and lines[-3].split()[5:] == ["0"] and lines[-1].split()[3:] == ["2", "3", "32768", "32768"]


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _fake_palette(k):
    """A stand-in palette handle whose K field (the first int) is k and whose host-side colour list is empty."""
    fake = C.create_string_buffer(8192)
    C.cast(fake, C.POINTER(C.c_int))[0] = k
    return fake


def _refused(lib, rc, code, *words):
    msg = lib.dp_last_error().decode()
    assert rc == code, (rc, msg)
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                # (the product library spells out no status name)
    for w in words:
        assert w in msg, (w, msg)


def test_idiff_refusals(lib):
    fn = "dp_idiff_u8"
    keep = _fake_palette(16)
    taps, divisor = ir.KERNELS["jjn"]
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))   # exactly n_taps each
    ok = dict(i=0x1001, o=0x2000003, n=3, h=4, w=5, pal=C.cast(keep, C.c_void_p), dx=dx.ctypes.data, dy=dy.ctypes.data, wt=wt.ctypes.data,
              nt=len(taps), d=divisor, s=128, ws=0x3000000, wsb=1 << 20)          # the device addresses are never dereferenced

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_idiff_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["pal"], v["dx"], v["dy"], v["wt"], v["nt"], v["d"], v["s"], v["ws"],
                               v["wsb"], None)

    def arr(values):
        a = np.array(values, np.int32)
        call.keep.append(a)
        return a.ctypes.data
    call.keep = []

    for bad in (dict(i=None), dict(o=None), dict(ws=None), dict(pal=None), dict(dx=None), dict(dy=None), dict(wt=None), dict(h=0), dict(w=0),
                dict(h=-1), dict(w=-7), dict(n=-1), dict(h=65536, w=65536)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for nt in (0, -1, 13):
        _refused(lib, call(nt=nt), 1, fn, "n_taps")
    for d in (0, -48):
        _refused(lib, call(d=d), 1, fn, "divisor")
    for s in (-1, 257, 1000, -256):
        _refused(lib, call(s=s), 1, fn, "strength256")
    for bad_dx, bad_dy in (([0], [0]), ([-1], [0]), ([3], [1]), ([-3], [1]), ([0], [3]), ([1], [-1])):
        _refused(lib, call(dx=arr(bad_dx), dy=arr(bad_dy), nt=1), 1, fn, "tap outside")
    _refused(lib, call(dx=arr([1, 1]), dy=arr([0, 0]), nt=2), 1, fn, "twice")
    _refused(lib, call(wt=arr([-1] + [0] * 11)), 1, fn, "negative weight")
    _refused(lib, call(d=47), 1, fn, "more than the divisor")
    _refused(lib, call(o=ok["i"]), 1, fn, "in_dev")
    for ws in (0x3000001, 0x3000008):
        _refused(lib, call(ws=ws), 1, fn, "16-byte aligned")
    for n in (3, 0):                                                    # the palette is checked before "nothing to do"
        big = _fake_palette(257)
        _refused(lib, call(pal=C.cast(big, C.c_void_p), n=n), 2, fn, "256")   # DP_EUNSUPPORTED
    need = lib.dp_idiff_workspace_bytes(3, 4, 5)
    assert need == 3 * 32 * 5
    _refused(lib, call(wsb=need - 1), 5, fn, "workspace too small", str(need))   # DP_EWORKSPACE, before the table or a launch
    _refused(lib, call(wsb=0), 5, fn, "workspace too small")
    assert call(n=0) == 0 and call(n=0, i=None, o=None, ws=None, wsb=0) == 0    # nothing to do is not an error, and launches nothing
    _refused(lib, call(n=0, nt=13), 1, fn, "n_taps")                    # ... but a bad argument still is one


# ---------------------------------------------------------------------------------------------------- the statement
BW = np.array([[0, 0, 0], [255, 255, 255]], np.float32)


def test_strength_zero_is_the_nearest_only_image(orc):
    rs = np.random.RandomState(3)
    pal = rs.randint(0, 256, (16, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = rs.randint(0, 256, (19, 23, 3)).astype(np.uint8)
    lut = rs.permutation(256).astype(np.uint8)
    for name in ("floyd_steinberg", "jjn", "atkinson"):
        taps, divisor = ir.KERNELS[name]
        assert np.array_equal(ir.idiff_u8(orc, img, pal, outc, None, taps, divisor, 0), orc.ordered_u8(img, pal, outc, None, "none"))
        assert np.array_equal(ir.idiff_u8(orc, img, pal, outc, lut, taps, divisor, 0), orc.ordered_u8(lut[img], pal, outc, None, "none"))


@pytest.mark.parametrize("name", sorted(ir.KERNELS))
def test_accumulator_fits_the_bound_on_random_input(orc, name):
    """|acc| <= 4080 * sum q_k / 65536 <= 4080: noise and saturated blocks, a black / white palette (the largest errors) and 16 colours."""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (40, 40, 3)).astype(np.uint8)
    img[:20, :20] = rs.randint(0, 2, (20, 20, 1)) * 255
    taps, divisor = ir.KERNELS[name]
    pal16 = rs.randint(0, 256, (16, 3)).astype(np.float32)
    for pal in (BW, pal16):
        _, big = ir.idiff_indices(orc, img, pal, pal.astype(np.uint8), None, taps, divisor, 256, want_acc=True)
        print(f"{name}, {len(pal)} colours: max |acc| {big}")
        assert 0 < big <= 4080, big


@pytest.mark.parametrize("name", ["floyd_steinberg", "jjn", "stucki", "sierra_lite", "burkes", "sierra", "sierra_two_row"])
@pytest.mark.parametrize("grey", [100, 128, 200])
def test_flat_greys_keep_their_mean(orc, name, grey):
    """The variants that diffuse the full error reproduce a flat grey with a black / white palette: the mean over rows and columns
    8.. of a 48 x 48 frame is within 1.0 level (0.65 was measured for the first four; Atkinson drops a quarter by design)."""
    taps, divisor = ir.KERNELS[name]
    assert sum(wt for _, _, wt in taps) == divisor
    img = np.full((48, 48, 3), grey, np.uint8)
    out = ir.idiff_u8(orc, img, BW, BW.astype(np.uint8), None, taps, divisor, 256)
    mean = float(out[8:, 8:].astype(np.float64).mean())
    print(f"{name}, grey {grey}: mean {mean:.3f}")
    assert abs(mean - grey) <= 1.0


def test_palette_colours_come_back_unchanged(orc):
    rs = np.random.RandomState(6)
    pal = rs.randint(0, 256, (8, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = outc[rs.randint(0, 8, (21, 18))]
    taps, divisor = ir.KERNELS["stucki"]
    assert np.array_equal(ir.idiff_u8(orc, img, pal, outc, None, taps, divisor, 256), img)   # e stays 0 everywhere


def test_statement_under_the_metric_differs_from_rgb(orc):
    import metric_ref as mr
    rs = np.random.RandomState(8)
    pal = rs.randint(0, 256, (16, 3)).astype(np.float32)
    img = rs.randint(0, 256, (12, 14, 3)).astype(np.uint8)
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    a = ir.idiff_indices(orc, img, pal, pal.astype(np.uint8), None, taps, divisor, 256)
    b = ir.idiff_indices(mr.NearestAdapter("oklab"), img, pal, pal.astype(np.uint8), None, taps, divisor, 256)
    assert (a != b).any()
    assert np.array_equal(ir.idiff_indices(mr.NearestAdapter("oklab"), img, pal, pal.astype(np.uint8), None, taps, divisor, 0),
                          mr.top2(img, pal, "oklab")[0])


# ---------------------------------------------------------------------------------------------------- Python surface
def test_strategy_metadata_and_parameters():
    from dither_pie_amd import dithering_lib as d
    S = d.IntegerErrorDiffusionDitherStrategy
    assert "IntegerErrorDiffusionDitherStrategy" in d.__all__ and issubclass(S, d.BaseDitherStrategy)
    info = S.get_parameter_info()
    assert list(info) == ["variant", "strength"]
    assert info["variant"]["type"] == "choice" and sorted(info["variant"]["choices"]) == sorted(ir.KERNELS) and info["variant"]["default"] == "floyd_steinberg"
    assert info["strength"]["type"] == "float" and (info["strength"]["min"], info["strength"]["max"], info["strength"]["default"]) == (0.0, 1.0, 1.0)
    s = S()
    assert s.get_current_parameters() == {"variant": "floyd_steinberg", "strength": 1.0}
    assert s._settings() == (ir.KERNELS["floyd_steinberg"][0], 16, 256)
    assert S("jjn", 0.3)._settings() == (ir.KERNELS["jjn"][0], 48, 77)
    assert S("stucki", 0)._settings()[2] == 0
    assert S("no_such_variant")._settings() == s._settings()            # the reference's fallback for an unknown name
    for bad in (dict(variant=4), dict(variant=None), dict(variant=("jjn",)), dict(strength=1.01), dict(strength=-0.01),
                dict(strength=float("nan")), dict(strength="x")):
        with pytest.raises(ValueError):
            S(**bad)._settings()
    assert not isinstance(s, d.ORDERED_STRATEGIES)                      # errors cross band edges
    assert not hasattr(d.DitherMode, "INTEGER_ERROR_DIFFUSION") and len(d.DitherMode) == 13
    with pytest.raises(ValueError, match="non-empty"):
        s.dither(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.float32), (0, 5))
    with pytest.raises(ValueError, match="256 colours"):
        s.dither(np.zeros((4, 3), np.float32), np.zeros((257, 3), np.float32), (2, 2))
    with pytest.raises(ValueError, match="cannot be tiled"):
        s._run(None, None, y0=1)
    with pytest.raises(ValueError, match="cannot be tiled"):
        s._run(None, None, x0=3)


def test_image_ditherer_takes_the_instance_under_either_metric():
    from dither_pie_amd import dithering_lib as d, sharding
    s = d.IntegerErrorDiffusionDitherStrategy("sierra", 0.25)
    for metric in ("rgb", "oklab"):
        dith = d.ImageDitherer(num_colors=8, dither_mode=s, palette=[(0, 0, 0), (255, 255, 255)], dither_params={"ignored": 1}, metric=metric)
        assert dith._get_dither_strategy(dith.dither_mode) is s
        assert dith._check_metric(s) == metric                          # the scan that takes a metric palette
        back = pickle.loads(pickle.dumps(dith))
        assert isinstance(back.dither_mode, d.IntegerErrorDiffusionDitherStrategy) and back.metric == metric
        assert (back.dither_mode.variant, back.dither_mode.strength, back.palette) == ("sierra", 0.25, dith.palette)
        with pytest.raises(ValueError, match="does not shard"):
            sharding.dither_band(dith, np.zeros((4, 4, 3), np.uint8), 0)
    assert isinstance(s, d._METRIC_STRATEGIES)
    with pytest.raises(ValueError, match="IntegerErrorDiffusionDitherStrategy"):    # ... and the message for the others names it
        d.ImageDitherer(dither_mode=d.DitherMode.ERROR_DIFFUSION, palette=[(0, 0, 0)], metric="oklab")._palette_on_device(
            d.ErrorDiffusionDitherStrategy())
    with pytest.raises(ValueError, match="use_gamma"):
        d.ImageDitherer(dither_mode=s, palette=[(0, 0, 0)], metric="oklab", use_gamma=True)
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy(d.IntegerErrorDiffusionDitherStrategy)   # the class is not an instance


def test_backend_argument_errors_come_before_the_device():
    from dither_pie_amd import backend

    class P:
        K = 16
    fs, d = ir.KERNELS["floyd_steinberg"]
    for taps, dv, s, word in ((fs, d, -1, "strength256"), (fs, d, 257, "strength256"), (fs, d, 0.5, "strength256"), (fs, 0, 256, "divisor"),
                              (fs, 16.0, 256, "divisor"), ([], d, 256, "taps"), (fs * 4, 64, 256, "taps"), ([(0, 0, 1)], 1, 256, "outside"),
                              ([(-1, 0, 1)], 1, 256, "outside"), ([(0, 3, 1)], 1, 256, "outside"), ([(3, 1, 1)], 1, 256, "outside"),
                              ([(1, 0, 1), (1, 0, 2)], 4, 256, "twice"), ([(1, 0, -1)], 4, 256, "negative"), (fs, 15, 256, "sum"),
                              ([(1, 0, 0.5)], 1, 256, "integers"), ([(1, 0)], 1, 256, "triples"), (7, 1, 256, "triples")):
        with pytest.raises(ValueError, match=word):
            backend.idiff(None, P(), taps, dv, s)
    P.K = 257
    with pytest.raises(ValueError, match="256 colours"):
        backend.idiff(None, P(), fs, d, 256)
