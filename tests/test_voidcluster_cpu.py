"""CPU tier of the void-and-cluster generator (include/ditherpie_hip_voidcluster.h, dithering_lib.VoidAndClusterDitherStrategy):
the agreement of the header, the ctypes table, the exported symbols and the memory-discipline module (the rule
tests/test_dotdiff_cpu.py keeps for its header); dp_void_cluster_host against the numpy statement tests/vac_ref.py and the
statement against its pins; properties of the matrices (permutation, convergence, minority spacing on the torus, spectrum);
the thresholds; the refusals of the three entry points, which happen before any HIP call; the Python surface; the host
statement under the sanitizers as a stand-alone program."""
import ctypes as C
import hashlib
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import vac_ref as vr
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")

# h, w, seed, sigma256 -> relaxation rounds, the first 16 hex digits of sha256 over the ranks as little-endian uint16
PINS = {
    (8, 8, 1, 384): (4, "3d0e6c07ad883f2a"),
    (16, 16, 1, 384): (13, "8101d7df080c056d"),
    (16, 24, 5, 256): (17, "f8fcfb43b6ef1930"),
    (13, 9, 3, 300): (7, "575d24604d25aebb"),
    (32, 32, 7, 768): (23, "0b5e68434a770245"),
    (64, 64, 42, 384): (155, "4c6c47909ccf1ed5"),
}
# ... and: a window wider than the matrix, a strip, the largest size
CASES = list(PINS) + [(8, 8, 1, 768), (128, 8, 2, 384), (128, 128, 3, 384)]
# the cases whose minority pattern is checked for spacing: both sizes >= 16, and the statement meets the condition.  It does
# not in two of the cases: 32 x 32 at sigma256 768 (under so wide a Gaussian neighbouring cells differ by little; one pair
# ends at distance 1) and 128 x 128 seed 3 (one diagonal pair among 1638 cells, distance sqrt 2)
SPACED = [(16, 16, 1, 384), (16, 24, 5, 256), (64, 64, 42, 384)]
QUALITY = [(32, s) for s in (1, 2, 3)] + [(64, s) for s in (1, 2, 3)]


@pytest.fixture(scope="module")
def statement():
    """The statement's rank matrix and relaxation record of every case, computed once."""
    out = {}
    for case in CASES:
        info = {}
        out[case] = (vr.ranks(*case, info=info), info)
    return out


@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_voidcluster.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_voidcluster_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_void_cluster_u16", "dp_void_cluster_host", "dp_thresholds_void_cluster"} == set(_lib.EXPORTS_VOIDCLUSTER)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
              | set(_lib.EXPORTS_PNG) | set(_lib.EXPORTS_PNG_DYN) | set(_lib.EXPORTS_PATTERN) | set(_lib.EXPORTS_PNG_FILE)
              | set(_lib.EXPORTS_DOTDIFF) | set(_lib.EXPORTS_CELLS))
    assert not set(_lib.EXPORTS_VOIDCLUSTER) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_VOIDCLUSTER[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == {"dp_void_cluster_u16"}
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
    for name in _lib.EXPORTS_VOIDCLUSTER:
        assert hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert lib.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: voidcluster.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_VOIDCLUSTER:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    limits = {k: int(re.search(rf"#define\s+DP_VOID_CLUSTER_{k}\s+(\d+)", _header_text()).group(1))
              for k in ("MIN_SIZE", "MAX_SIZE", "MIN_SIGMA256", "MAX_SIGMA256")}
    assert (limits["MIN_SIZE"], limits["MAX_SIZE"]) == backend.VOID_CLUSTER_SIZES == (vr.MIN_SIZE, vr.MAX_SIZE) == (8, 128)
    assert (limits["MIN_SIGMA256"], limits["MAX_SIGMA256"]) == backend.VOID_CLUSTER_SIGMA256 == (vr.MIN_SIGMA256, vr.MAX_SIGMA256) == (256, 768)


# ---------------------------------------------------------------------------------------------------- the statement and its pins
def test_statement_pins(statement):
    assert [vr.key(i, 1) for i in range(3)] == [0x688990c0, 0xd25b73e6, 0x123a4a88]
    assert [len(vr.weights(s)) - 1 for s in (256, 384, 512, 768)] == [29, 65, 116, 262]
    assert all(np.all(np.diff(vr.weights(s)) <= 0) for s in (256, 300, 384, 768))   # never rising: nothing follows the first zero
    assert int(vr.cell_weights(128, 128, 768).sum()) == 59295600 < 2 ** 31        # the largest energy there is
    for case, (rounds, digest) in PINS.items():
        r, info = statement[case]
        assert info["rounds"] == rounds, (case, info)
        assert hashlib.sha256(r.astype("<u2").tobytes()).hexdigest()[:16] == digest, case
    assert statement[(8, 8, 1, 384)][0][0].tolist() == [32, 48, 40, 56, 34, 50, 42, 58]


def test_wide_window_touches_every_cell_once():
    """8 x 8 at sigma256 768: the weights reach 16 cells, the matrix is 8 wide.  A cell's weights are those of the minimum
    image, each cell once: the sum is far below what a loop over +-16 offsets would add up."""
    T = vr.cell_weights(8, 8, 768)
    W = vr.weights(768)
    assert T[0, 0] == W[0] == 1 << 20 and T[4, 4] == W[32] and T[7, 1] == W[2] and T[3, 5] == W[9 + 9]
    assert (T > 0).all() and T.sum() < sum(int(W[a * a + b * b]) for a in range(-16, 17) for b in range(-16, 17) if a * a + b * b < len(W))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_host_entry_point_equals_the_statement(lib, statement, case):
    h, w, seed, s256 = case
    want, info = statement[case]
    got = np.full((h, w), 0xFFFF, np.uint16)
    assert lib.dp_void_cluster_host(got.ctypes.data, h, w, seed, s256) == 0, lib.dp_last_error()
    assert np.array_equal(got, want)
    assert sorted(want.reshape(-1).tolist()) == list(range(h * w))      # a permutation of 0 .. n-1
    assert info["converged"] and info["rounds"] < 4 * h * w             # the relaxation ends before its cap
    from dither_pie_amd import backend
    if h * w <= 4096:
        assert np.array_equal(backend.void_cluster_ranks_host(h, w, seed, s256 / 256), want)


@pytest.mark.parametrize("case", SPACED, ids=lambda c: "x".join(map(str, c)))
def test_minority_pattern_is_spaced_on_the_torus(statement, case):
    """The cells of rank < n / 10 (the prototype): no two within a minimum-image distance below 2, seam included."""
    h, w = case[:2]
    r = statement[case][0]
    ys, xs = np.nonzero(r < h * w / 10)
    for wrap in (False, True):
        dy, dx = np.abs(ys[:, None] - ys[None, :]), np.abs(xs[:, None] - xs[None, :])
        if wrap:
            dy, dx = np.minimum(dy, h - dy), np.minimum(dx, w - dx)
        d2 = dy * dy + dx * dx + (np.eye(len(ys), dtype=np.int64) << 40)
        assert d2.min() >= 4, (case, wrap, int(d2.min()))


@pytest.mark.parametrize("size, seed", QUALITY)
def test_spectrum_is_blue_at_every_grey_level(lib, size, seed):
    """Mean power below a quarter of Nyquist over mean power at all non-zero frequencies: at most 0.2 at each of five grey
    levels (the reference's generator gives 0.17 to 1.02, a random permutation 1.0) -- on the library's matrix."""
    r = np.empty((size, size), np.uint16)
    assert lib.dp_void_cluster_host(r.ctypes.data, size, size, seed, 384) == 0
    ratios = [vr.lowfreq(r.astype(np.int64), g) for g in vr.GREYS]
    print(size, seed, [round(v, 4) for v in ratios])
    assert max(ratios) <= 0.2, ratios
    rnd = np.random.RandomState(seed).permutation(size * size).reshape(size, size)
    assert min(vr.lowfreq(rnd, g) for g in vr.GREYS) > 0.5              # the measure tells the two apart


# ---------------------------------------------------------------------------------------------------- thresholds
def test_thresholds(statement):
    from dither_pie_amd import backend
    for case, (r, _) in statement.items():
        n = r.size
        L = min(n, 4096)
        t = vr.thresholds(r)
        assert t.dtype == np.float32 and t.shape == r.shape and (t > 0).all() and (t < 1).all(), case
        level = (r * L // n).reshape(-1)
        order = np.argsort(level, kind="stable")
        tl, ll = t.reshape(-1)[order], level[order]
        assert np.all(np.diff(tl)[np.diff(ll) > 0] > 0) and np.all(np.diff(tl)[np.diff(ll) == 0] == 0), case   # strictly increasing in the level
        assert np.array_equal(np.unique(level), np.arange(L)), case
        assert np.array_equal(backend.void_cluster_thresholds(r), t), case
    for h, w in ((16, 16), (32, 32), (64, 64), (128, 128)):                  # multiples of 2^-13: the integer form of the kernels
        t = vr.thresholds(np.arange(h * w).reshape(h, w)).astype(np.float64) * 8192
        assert np.array_equal(t, np.floor(t)) and t.min() >= 1 and t.max() <= 8191, (h, w)


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
def _refused(lib, rc, fn):
    msg = lib.dp_last_error().decode()
    assert rc == 1 and fn in msg, (rc, msg)                             # DP_EINVAL
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                 # (the product library spells out no status name)


BAD_SHAPES = (dict(h=7), dict(h=129), dict(w=7), dict(w=129), dict(h=0), dict(w=-8), dict(s=255), dict(s=769), dict(s=0), dict(s=-384))


def test_device_entry_point_refusals(lib):
    seeds = np.array([1, 2, 3], np.uint32)
    ok = dict(r=0x2000002, n=3, sd=seeds.ctypes.data, h=16, w=24, s=384)   # ranks_dev is never dereferenced

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_void_cluster_u16(v["r"], v["n"], v["sd"], v["h"], v["w"], v["s"], None)

    for bad in (dict(r=None), dict(sd=None), dict(n=-1)) + BAD_SHAPES:
        _refused(lib, call(**bad), "dp_void_cluster_u16")
    assert call(n=0) == 0 and call(n=0, r=None, sd=None) == 0           # nothing to do is not an error, and launches nothing
    _refused(lib, call(n=0, h=7), "dp_void_cluster_u16")                # ... but a bad argument still is one


def test_host_and_thresholds_entry_point_refusals(lib):
    out = np.full((16, 24), 0xABCD, np.uint16)
    handle = C.c_void_p(0x1234)
    for bad in (dict(r=None),) + BAD_SHAPES:
        v = dict(dict(r=out.ctypes.data, h=16, w=24, s=384), **bad)
        _refused(lib, lib.dp_void_cluster_host(v["r"], v["h"], v["w"], 5, v["s"]), "dp_void_cluster_host")
    assert (out == 0xABCD).all()
    for bad in (dict(o=None),) + BAD_SHAPES:
        v = dict(dict(o=C.byref(handle), h=16, w=24, s=384), **bad)
        _refused(lib, lib.dp_thresholds_void_cluster(v["h"], v["w"], 5, v["s"], None, v["o"]), "dp_thresholds_void_cluster")
    assert handle.value == 0x1234                                       # refused before any HIP call: nothing was made


# ---------------------------------------------------------------------------------------------------- Python surface
def test_backend_argument_errors_come_before_the_device():
    from dither_pie_amd import backend
    for h, w, sigma in ((7, 16, 1.5), (16, 129, 1.5), (16.0, 16, 1.5), ("16", 16, 1.5), (True, 16, 1.5), (16, 16, 0.99), (16, 16, 3.01),
                        (16, 16, "wide"), (16, 16, None), (16, 16, float("nan"))):
        for fn, seed in ((backend.void_cluster_ranks, [1]), (backend.void_cluster_ranks_host, 1), (backend.Thresholds.void_cluster, 1)):
            with pytest.raises(ValueError, match="void-and-cluster"):
                fn(h, w, seed, sigma)
    for seeds in ([1.5], "x", [[1, 2]]):
        with pytest.raises(ValueError, match="seeds"):
            backend.void_cluster_ranks(16, 16, seeds)
    with pytest.raises(ValueError, match="one seed"):
        backend.void_cluster_ranks_host(16, 16, [1, 2])
    assert backend._void_cluster_args(8, 128, 1.0) == (8, 128, 256) and backend._void_cluster_args(np.int64(9), 9, 3.0) == (9, 9, 768)
    assert backend._void_cluster_args(8, 8, 1.498)[2] == 383 and backend._void_cluster_args(8, 8, 1.5)[2] == 384


def test_strategy_metadata_parameters_and_pickling(monkeypatch):
    from dither_pie_amd import dithering_lib as d
    assert {"VoidAndClusterDitherStrategy", "generate_void_and_cluster"} <= set(d.__all__)
    assert issubclass(d.VoidAndClusterDitherStrategy, d.MatrixDitherStrategy) and isinstance(d.VoidAndClusterDitherStrategy(), d.ORDERED_STRATEGIES)
    info = d.VoidAndClusterDitherStrategy.get_parameter_info()
    assert list(info) == ["size", "seed", "sigma"]
    assert (info["size"]["type"], info["size"]["default"], info["size"]["min"], info["size"]["max"]) == ("int", 64, 8, 128)
    assert (info["seed"]["type"], info["seed"]["default"]) == ("int", 42)
    assert (info["sigma"]["type"], info["sigma"]["default"], info["sigma"]["min"], info["sigma"]["max"]) == ("float", 1.5, 1.0, 3.0)
    s = d.VoidAndClusterDitherStrategy()
    assert s.get_current_parameters() == {"size": 64, "seed": 42, "sigma": 1.5} == {k: v["default"] for k, v in info.items()}
    assert d._vac_settings(64, 42, 1.5) == (64, 64, 42, 384) and d._vac_settings((13, 9), -1, 1.0) == (13, 9, 0xFFFFFFFF, 256)
    for bad in (dict(size=7), dict(size=(8, 129)), dict(size=(8, 8, 8)), dict(size="64"), dict(size=64.0), dict(seed=1.5), dict(seed="x"),
                dict(sigma=0.5), dict(sigma=4), dict(sigma="x")):
        with pytest.raises(ValueError, match="void-and-cluster"):
            d.VoidAndClusterDitherStrategy(**bad)
        with pytest.raises(ValueError, match="void-and-cluster"):
            d.generate_void_and_cluster(**bad)
    assert not hasattr(d.DitherMode, "VOID_AND_CLUSTER") and "void" not in " ".join(m.value for m in d.DitherMode)
    assert "VoidAndClusterDitherStrategy" in d.ImageDitherer._get_dither_strategy.__doc__

    # the matrix is made lazily, is the statement's, and does not travel in a pickle; without a device the host statement makes it
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    s = d.VoidAndClusterDitherStrategy((16, 24), 5, 1.0)
    assert s._matrix is None
    want = vr.thresholds(vr.ranks(16, 24, 5, 256))
    m = s.threshold_matrix
    assert m.dtype == np.float32 and m.tobytes() == want.tobytes() and s.threshold_matrix is m
    assert d.generate_void_and_cluster((16, 24), 5, 1.0).tobytes() == want.tobytes()
    assert d.generate_void_and_cluster(8, seed=1).tobytes() == vr.thresholds(vr.ranks(8, 8, 1, 384)).tobytes()
    back = pickle.loads(pickle.dumps(s))
    assert back._matrix is None and back.get_current_parameters() == {"size": (16, 24), "seed": 5, "sigma": 1.0}
    dith = d.ImageDitherer(num_colors=2, dither_mode=s, palette=[(0, 0, 0), (255, 255, 255)], dither_params={"ignored": 1})
    assert dith._get_dither_strategy(dith.dither_mode) is s
    back = pickle.loads(pickle.dumps(dith))
    assert isinstance(back.dither_mode, d.VoidAndClusterDitherStrategy) and back.dither_mode._matrix is None and back.dither_mode.seed == 5
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy(d.VoidAndClusterDitherStrategy)   # the class is not an instance


# ---------------------------------------------------------------------------------------------------- sanitizers
def test_host_statement_under_the_sanitizers(statement, tmp_path):
    """The stand-alone harness (csrc/host_sanitize.cpp, built with -fsanitize=address,undefined; a program with its own main,
    nothing preloaded) runs vac_generate and vac_thresholds on buffers of exactly h * w entries and prints what they give."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    cases = [c for c in CASES if c[0] * c[1] <= 1024]
    assert (8, 8, 1, 768) in cases and (13, 9, 3, 300) in cases and (128, 8, 2, 384) in cases
    with open(tmp_path / "cases.bin", "wb") as f:
        for case in cases:
            f.write(np.array(case, np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "host_asan"), "voidcluster", str(tmp_path / "cases.bin"), str(len(cases))], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    ranks = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ranks ")]
    thr = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("thr ")]
    assert len(ranks) == len(thr) == len(cases)
    for c, case in enumerate(cases):
        want, info = statement[case]
        assert int(ranks[c][1]) == c and int(ranks[c][2]) == info["rounds"], case
        assert np.array_equal(np.array(ranks[c][3:], np.int64), want.reshape(-1)), case
        bits = np.array([int(v, 16) for v in thr[c][2:]], np.uint32)
        assert int(thr[c][1]) == c and np.array_equal(bits, vr.thresholds(want).reshape(-1).view(np.uint32)), case
    bad = tmp_path / "bad.bin"
    bad.write_bytes(np.array([8, 7, 1, 384], np.int32).tobytes())
    assert subprocess.run([os.path.join(CSRC, "build", "host_asan"), "voidcluster", str(bad), "1"], capture_output=True, env=env).returncode == 2
