"""CPU tier of dot diffusion (include/ditherpie_hip_dotdiff.h, dithering_lib.DotDiffusionDitherStrategy): the agreement of the
header, the ctypes table, the exported symbols and the memory-discipline module (the rule tests/test_pattern_cpu.py keeps
for its header); the default matrix; dp_dotdiff_reach (host code) against the longest-path definition of
tests/dotdiff_ref.py; the two properties of levels() the kernel's schedule rests on; properties of the numpy statement that
follow from the definition alone; the refusals of dp_dotdiff_u8, which happen before any HIP call; the Python surface."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import dotdiff_ref as dr
import pattern_ref as pr
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_dotdiff.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_dotdiff_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_dotdiff_reach", "dp_dotdiff_u8"} == set(_lib.EXPORTS_DOTDIFF)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
              | set(_lib.EXPORTS_PNG) | set(_lib.EXPORTS_PNG_DYN) | set(_lib.EXPORTS_PATTERN) | set(_lib.EXPORTS_PNG_FILE))
    assert not set(_lib.EXPORTS_DOTDIFF) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_DOTDIFF[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == {"dp_dotdiff_u8"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version():
    import subprocess
    from dither_pie_amd import _lib, backend
    L = _lib.load()
    for name in _lib.EXPORTS_DOTDIFF:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: dotdiff.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_DOTDIFF:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    assert int(re.search(r"#define\s+DP_DOTDIFF_MAX_REACH\s+(\d+)", _header_text()).group(1)) == backend.DOTDIFF_MAX_REACH == dr.MAX_REACH == 16
    with open(os.path.join(ROOT, "dither_pie_amd", "csrc", "dotdiff.hip")) as f:
        assert int(re.search(r"constexpr int kDotTile = (\d+);", f.read()).group(1)) == backend.DOTDIFF_TILE


def test_default_matrix_is_the_headers():
    from dither_pie_amd.dithering_lib import DotDiffusionDitherStrategy as S
    rows = re.findall(r"^ \*((?:\s+\d+){8})\s*$", _header_text(), flags=re.M)
    assert len(rows) == 8
    header = np.array([[int(v) for v in r.split()] for r in rows])
    assert np.array_equal(header, dr.KNUTH) and np.array_equal(np.array(S.MATRICES["knuth"]), dr.KNUTH)
    assert sorted(dr.KNUTH.reshape(-1).tolist()) == list(range(64))
    assert dr.reach(dr.KNUTH) == 14
    lv = dr.levels(dr.KNUTH)                                            # the barons: the cells no neighbour exceeds
    barons = [int(dr.KNUTH[y, x]) for y in range(8) for x in range(8)
              if all(dr.KNUTH[(y + dy) % 8, (x + dx) % 8] < dr.KNUTH[y, x] for dy, dx, _ in dr.NEIGHBOURS)]
    assert sorted(barons) == [62, 63] and lv.max() == 14


# ---------------------------------------------------------------------------------------------------- reach and levels
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _reach(lib, M):
    a = np.ascontiguousarray(M, np.uint8)
    return lib.dp_dotdiff_reach(a.ctypes.data, a.shape[0])


def test_library_reach_equals_the_definition(lib):
    assert _reach(lib, dr.KNUTH) == 14
    for m in (2, 4, 8):
        assert _reach(lib, pr.bayer_rank(m)) == dr.reach(pr.bayer_rank(m)) == 3
    rs = np.random.RandomState(77)
    got = {4: [], 8: [], 16: []}
    for m in got:
        for _ in range(200):
            M = rs.permutation(m * m).reshape(m, m)
            r = _reach(lib, M)
            assert r == dr.reach(M), (m, M.tolist())
            got[m].append(r)
    assert max(got[16]) > 16 > min(got[8])                              # both sides of the limit occur
    twice = dr.KNUTH.copy()
    twice[3, 3] = twice[0, 0]
    assert _reach(lib, twice) == -1 and lib.dp_dotdiff_reach(None, 8) == -1
    nine = np.arange(9, dtype=np.uint8)
    assert lib.dp_dotdiff_reach(nine.ctypes.data, 3) == -1
    for m in (0, 1, 3, 5, 32, -8):
        assert lib.dp_dotdiff_reach(np.arange(64, dtype=np.uint8).ctypes.data, m) == -1
    high = np.arange(16, dtype=np.uint8)
    high[5] = 16                                                        # a class beyond m*m - 1
    assert lib.dp_dotdiff_reach(high.ctypes.data, 4) == -1


@pytest.mark.parametrize("m", [2, 4, 8, 16])
def test_levels_make_a_schedule(m):
    rs = np.random.RandomState(100 + m)
    for M in [rs.permutation(m * m).reshape(m, m) for _ in range(20)] + ([dr.KNUTH] if m == 8 else []):
        lv = dr.levels(M)
        assert lv.min() == 0 and set(np.unique(lv).tolist()) == set(range(lv.max() + 1))
        for dy, dx, _ in dr.NEIGHBOURS:
            nb_cls, nb_lv = np.roll(M, (dy, dx), (0, 1)), np.roll(lv, (dy, dx), (0, 1))
            assert (nb_lv != lv).all()                                  # neighbouring cells never share a level
            assert (lv[nb_cls < M] > nb_lv[nb_cls < M]).all()           # a cell's level exceeds that of every lower-class neighbour


# ---------------------------------------------------------------------------------------------------- the statement
BW = np.array([[0, 0, 0], [255, 255, 255]], np.float32)


@pytest.mark.parametrize("grey", [16, 64, 128, 200])
def test_flat_greys_keep_their_mean(orc, grey):
    img = np.full((64, 64, 3), grey, np.uint8)
    idx, big = dr.dotdiff_indices(orc, img, BW, BW.astype(np.uint8), None, dr.KNUTH, 256, want_acc=True)
    white = float(idx.mean())
    print(f"grey {grey}: white fraction {white:.4f}, target {grey / 255:.4f}, max |acc| {big}")
    assert abs(white - grey / 255) <= 0.01
    assert big <= 32640
    near = orc.ordered_u8(img, BW, BW.astype(np.uint8), None, "none")
    assert np.array_equal(dr.dotdiff_u8(orc, img, BW, BW.astype(np.uint8), None, dr.KNUTH, 0), near)


def test_strength_zero_is_the_nearest_only_image(orc):
    rs = np.random.RandomState(3)
    pal = rs.randint(0, 256, (16, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = rs.randint(0, 256, (19, 23, 3)).astype(np.uint8)
    lut = rs.permutation(256).astype(np.uint8)
    for M in (dr.KNUTH, pr.bayer_rank(4), rs.permutation(256).reshape(16, 16)):
        assert np.array_equal(dr.dotdiff_u8(orc, img, pal, outc, None, M, 0), orc.ordered_u8(img, pal, outc, None, "none"))
        assert np.array_equal(dr.dotdiff_u8(orc, img, pal, outc, lut, M, 0), orc.ordered_u8(lut[img], pal, outc, None, "none"))


def test_accumulator_bound_on_the_harshest_input(orc):
    """Black / white palette, noise and saturated blocks, every strength: |acc| stays within what an int16 holds."""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (40, 48, 3)).astype(np.uint8)
    img[:20, :24] = rs.randint(0, 2, (20, 24, 1)) * 255
    for M in (dr.KNUTH, pr.bayer_rank(2), rs.permutation(64).reshape(8, 8)):
        for s in (77, 256):
            _, big = dr.dotdiff_indices(orc, img, BW, BW.astype(np.uint8), None, M, s, want_acc=True)
            assert 0 < big <= 32640, big


def test_palette_colours_come_back_unchanged(orc):
    rs = np.random.RandomState(6)
    pal = rs.randint(0, 256, (8, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = outc[rs.randint(0, 8, (21, 18))]
    assert np.array_equal(dr.dotdiff_u8(orc, img, pal, outc, None, dr.KNUTH, 256), img)   # e stays 0 everywhere


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
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


def test_dotdiff_refusals(lib):
    fn = "dp_dotdiff_u8"
    keep = _fake_palette(16)
    knuth = np.ascontiguousarray(dr.KNUTH, np.uint8)
    ok = dict(i=0x1001, o=0x2000003, n=3, h=4, w=5, pal=C.cast(keep, C.c_void_p), c=knuth.ctypes.data, m=8, s=128)   # never dereferenced

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_dotdiff_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["pal"], v["c"], v["m"], v["s"], None)

    for bad in (dict(i=None), dict(o=None), dict(pal=None), dict(c=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-7), dict(n=-1),
                dict(h=65536, w=65536)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for m in (0, 1, 3, 5, 6, 32, -2):
        _refused(lib, call(m=m), 1, fn, "class matrix")
    twice = knuth.copy()
    twice[7, 7] = twice[0, 0]
    _refused(lib, call(c=twice.ctypes.data), 1, fn, "permutation")
    _refused(lib, call(c=knuth.ctypes.data, m=4), 1, fn, "permutation")  # the first 16 bytes of the 8 x 8 matrix are no 4 x 4 one
    for s in (-1, 257, 1000, -256):
        _refused(lib, call(s=s), 1, fn, "strength256")
    _refused(lib, call(o=ok["i"]), 1, fn, "in_dev")
    for n in (3, 0):                                                    # the palette is checked before "nothing to do"
        big = _fake_palette(257)
        _refused(lib, call(pal=C.cast(big, C.c_void_p), n=n), 2, fn, "256")   # DP_EUNSUPPORTED
    rs = np.random.RandomState(2032)
    far = next(c for c in (np.ascontiguousarray(rs.permutation(64).reshape(8, 8), np.uint8) for _ in range(2000)) if dr.reach(c) == 17)
    for n in (3, 0):
        _refused(lib, call(c=far.ctypes.data, n=n), 2, fn, "reach 17")
    assert call(n=0) == 0 and call(n=0, i=None, o=None) == 0            # nothing to do is not an error, and launches nothing
    _refused(lib, call(n=0, m=3), 1, fn, "class matrix")                # ... but a bad argument still is one


# ---------------------------------------------------------------------------------------------------- Python surface
def test_strategy_metadata_and_parameters():
    from dither_pie_amd import dithering_lib as d
    assert "DotDiffusionDitherStrategy" in d.__all__ and issubclass(d.DotDiffusionDitherStrategy, d.BaseDitherStrategy)
    info = d.DotDiffusionDitherStrategy.get_parameter_info()
    assert list(info) == ["matrix", "strength"]
    assert info["matrix"]["type"] == "choice" and info["matrix"]["choices"] == ["knuth"] and info["matrix"]["default"] == "knuth"
    assert info["strength"]["type"] == "float" and (info["strength"]["min"], info["strength"]["max"], info["strength"]["default"]) == (0.0, 1.0, 1.0)
    s = d.DotDiffusionDitherStrategy()
    assert s.get_current_parameters() == {"matrix": "knuth", "strength": 1.0}
    classes, s256 = s._settings()
    assert classes.dtype == np.uint8 and np.array_equal(classes, dr.KNUTH) and s256 == 256
    classes, s256 = d.DotDiffusionDitherStrategy(pr.bayer_rank(4).tolist(), 0.3)._settings()
    assert np.array_equal(classes, pr.bayer_rank(4)) and s256 == 77
    assert d.DotDiffusionDitherStrategy("knuth", 0)._settings()[1] == 0
    twice = dr.KNUTH.copy()
    twice[1, 1] = twice[0, 0]
    for bad in (dict(matrix="bayer"), dict(matrix=4), dict(matrix=twice), dict(matrix=np.arange(9).reshape(3, 3)),
                dict(matrix=dr.KNUTH.astype(np.float32)), dict(matrix=np.arange(64)), dict(strength=1.01), dict(strength=-0.01),
                dict(strength=float("nan")), dict(strength="x")):
        with pytest.raises(ValueError):
            d.DotDiffusionDitherStrategy(**bad)._settings()
    assert not isinstance(d.DotDiffusionDitherStrategy(), d.ORDERED_STRATEGIES)   # errors cross band edges
    assert not hasattr(d.DitherMode, "DOT_DIFFUSION") and len(d.DitherMode) == len({m.value for m in d.DitherMode})
    with pytest.raises(ValueError, match="non-empty"):
        s.dither(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.float32), (0, 5))
    with pytest.raises(ValueError, match="256 colours"):
        s.dither(np.zeros((4, 3), np.float32), np.zeros((257, 3), np.float32), (2, 2))


def test_image_ditherer_takes_the_instance():
    from dither_pie_amd import dithering_lib as d
    s = d.DotDiffusionDitherStrategy(pr.bayer_rank(4), 0.25)
    dith = d.ImageDitherer(num_colors=8, dither_mode=s, palette=[(0, 0, 0), (255, 255, 255)], dither_params={"ignored": 1})
    assert dith._get_dither_strategy(dith.dither_mode) is s
    back = pickle.loads(pickle.dumps(dith))
    assert isinstance(back.dither_mode, d.DotDiffusionDitherStrategy) and back.dither_mode.strength == 0.25
    assert np.array_equal(back.dither_mode.matrix, pr.bayer_rank(4)) and back.palette == dith.palette
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy(d.DotDiffusionDitherStrategy)   # the class is not an instance


def test_backend_argument_errors_come_before_the_device():
    from dither_pie_amd import backend

    class P:
        K = 16
    twice = dr.KNUTH.copy()
    twice[1, 1] = twice[0, 0]
    for M in (3, "knuth", np.arange(9).reshape(3, 3), twice, dr.KNUTH.astype(np.float64), np.arange(1024).reshape(32, 32)):
        with pytest.raises(ValueError, match="class matrix"):
            backend.dotdiff(None, P(), M, 128)
        with pytest.raises(ValueError, match="class matrix"):
            backend.dotdiff_reach(M)
    for s in (-1, 257, 0.5):
        with pytest.raises(ValueError, match="strength256"):
            backend.dotdiff(None, P(), dr.KNUTH, s)
    rs = np.random.RandomState(2032)
    far = next(c for c in (rs.permutation(64).reshape(8, 8) for _ in range(2000)) if dr.reach(c) == 17)
    assert backend.dotdiff_reach(far) == 17 and backend.dotdiff_reach(dr.KNUTH) == 14
    with pytest.raises(ValueError, match="reach 17"):
        backend.dotdiff(None, P(), far, 128)
    P.K = 257
    with pytest.raises(ValueError, match="256 colours"):
        backend.dotdiff(None, P(), dr.KNUTH, 128)
