"""CPU tier of pattern (Knoll) dithering (include/ditherpie_hip_pattern.h, dithering_lib.PatternDitherStrategy): the rank
matrix; properties of the numpy statement (tests/pattern_ref.py) that follow from the definition alone; the agreement of the
header, the ctypes table, the exported symbols and the memory-discipline module (the rule tests/test_scenes_cpu.py keeps for
its header); the refusals of dp_pattern_u8 / dp_pattern_prepare, which happen before any HIP call; the strategy's metadata
and the instance hook of ImageDitherer.  (The refusal of a palette VALUE outside [0, 255] needs a real dp_palette, which
needs a device -- a stand-in handle cannot carry the host-side colour list --: tests/test_gpu_pattern_memory.py has it.)"""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import pattern_ref as pr
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("m", [2, 4, 8])
def test_rank_matrix_is_a_permutation(m):
    b = pr.bayer_rank(m)
    assert b.shape == (m, m) and sorted(b.reshape(-1).tolist()) == list(range(m * m))
    assert b[0, 0] == 0
    if m == 2:
        assert b.tolist() == [[0, 2], [3, 1]]
    else:
        half = pr.bayer_rank(m // 2)
        h = m // 2
        assert np.array_equal(b[:h, :h], 4 * half) and np.array_equal(b[:h, h:], 4 * half + 2)
        assert np.array_equal(b[h:, :h], 4 * half + 3) and np.array_equal(b[h:, h:], 4 * half + 1)


def _rnd(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_strength_zero_is_the_nearest_only_image(orc):
    pal = np.random.RandomState(3).randint(0, 256, (16, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = _rnd(4, 9, 13)
    want = orc.ordered_u8(img, pal, outc, None, "none")
    for m in (2, 4, 8):
        assert np.array_equal(pr.pattern_u8(orc, img, pal, outc, None, m, 0), want)
        assert np.array_equal(pr.pattern_u8(orc, img, pal, outc, None, m, 0, y0=3, x0=5), want)


def test_one_colour_gives_index_zero(orc):
    pal = np.array([[10, 200, 30]], np.float32)
    idx = pr.pattern_indices(orc, _rnd(5, 7, 5), pal, pal.astype(np.uint8), None, 4, 256)
    assert idx.shape == (7, 5) and not idx.any()


def test_palette_colours_come_back_unchanged(orc):
    pal = np.random.RandomState(6).randint(0, 256, (8, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = outc[np.random.RandomState(7).randint(0, 8, (11, 6))]
    for m, s in ((2, 256), (4, 128), (8, 77)):
        assert np.array_equal(pr.pattern_u8(orc, img, pal, outc, None, m, s), img)   # e stays 0: every candidate is the pixel


def test_offsets_shift_the_pattern(orc):
    pal = np.random.RandomState(8).randint(0, 256, (5, 3)).astype(np.float32)
    outc = pal.astype(np.uint8)
    img = _rnd(9, 12, 14)
    whole = pr.pattern_u8(orc, img, pal, outc, None, 4, 200)
    assert np.array_equal(pr.pattern_u8(orc, img[3:, 5:], pal, outc, None, 4, 200, y0=3, x0=5), whole[3:, 5:])


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_functions():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_pattern.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_pattern_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_pattern_prepare", "dp_pattern_table_bytes", "dp_pattern_u8"} == set(_lib.EXPORTS_PATTERN)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
              | set(_lib.EXPORTS_PNG) | set(_lib.EXPORTS_PNG_DYN))
    assert not set(_lib.EXPORTS_PATTERN) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_PATTERN[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    # the device entry points: whatever takes a *_dev pointer, and dp_pattern_prepare, which launches the table build
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)} | {"dp_pattern_prepare"}
    assert with_dev == {"dp_pattern_u8", "dp_pattern_prepare"}
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
    from dither_pie_amd import _lib
    L = _lib.load()
    for name in _lib.EXPORTS_PATTERN:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: pattern.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_PATTERN:
            assert re.search(rf"\bT {name}\b", sym), (path, name)


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


def test_pattern_refusals(lib):
    fn = "dp_pattern_u8"
    keep = _fake_palette(16)
    ok = dict(i=0x1001, o=0x2000003, n=3, h=4, w=5, y0=0, x0=0, pal=C.cast(keep, C.c_void_p), m=4, s=128)   # never dereferenced

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_pattern_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["y0"], v["x0"], v["pal"], v["m"], v["s"], None)

    for bad in (dict(i=None), dict(o=None), dict(pal=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-7), dict(n=-1), dict(y0=-1),
                dict(x0=-1), dict(h=65536, w=65536), dict(y0=2 ** 30), dict(x0=2 ** 30)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for m in (0, 1, 3, 5, 6, 16, -2):
        _refused(lib, call(m=m), 1, fn, "matrix")
    for s in (-1, 257, 1000, -256):
        _refused(lib, call(s=s), 1, fn, "strength256")
    for n in (3, 0):                                                    # the palette is checked before "nothing to do"
        big = _fake_palette(257)
        _refused(lib, call(pal=C.cast(big, C.c_void_p), n=n), 2, fn, "256")   # DP_EUNSUPPORTED
    assert call(n=0) == 0 and call(n=0, i=None, o=None) == 0            # nothing to do is not an error, and launches nothing
    _refused(lib, call(n=0, m=3), 1, fn, "matrix")                      # ... but a bad argument still is one


def test_prepare_refusals_and_table_bytes(lib):
    _refused(lib, lib.dp_pattern_prepare(None), 1, "dp_pattern_prepare", "NULL")
    big = _fake_palette(1024)
    _refused(lib, lib.dp_pattern_prepare(C.cast(big, C.c_void_p)), 2, "dp_pattern_prepare", "256")
    assert lib.dp_pattern_table_bytes(None) == 0 and lib.dp_pattern_table_bytes(C.cast(big, C.c_void_p)) == 0
    ok = _fake_palette(256)
    assert lib.dp_pattern_table_bytes(C.cast(ok, C.c_void_p)) == (1 << 24) + 3 * 1024


# ---------------------------------------------------------------------------------------------------- Python surface
def test_strategy_metadata_and_parameters():
    from dither_pie_amd import dithering_lib as d
    assert "PatternDitherStrategy" in d.__all__ and issubclass(d.PatternDitherStrategy, d.BaseDitherStrategy)
    info = d.PatternDitherStrategy.get_parameter_info()
    assert list(info) == ["matrix", "strength"]
    assert info["matrix"]["type"] == "choice" and info["matrix"]["choices"] == ["2x2", "4x4", "8x8"] and info["matrix"]["default"] == "4x4"
    assert info["strength"]["type"] == "float" and (info["strength"]["min"], info["strength"]["max"], info["strength"]["default"]) == (0.0, 1.0, 0.5)
    s = d.PatternDitherStrategy()
    assert s.get_current_parameters() == {"matrix": "4x4", "strength": 0.5}
    s = d.PatternDitherStrategy(matrix="8x8", strength=0.3)
    assert s.get_current_parameters() == {"matrix": "8x8", "strength": 0.3} and s._settings() == (8, 77)
    assert d.PatternDitherStrategy("2x2", 1.0)._settings() == (2, 256) and d.PatternDitherStrategy("2x2", 0)._settings() == (2, 0)
    for bad in (dict(matrix="3x3"), dict(matrix=4), dict(strength=1.01), dict(strength=-0.01), dict(strength=float("nan")), dict(strength="x")):
        with pytest.raises(ValueError):
            d.PatternDitherStrategy(**bad)._settings()
    assert isinstance(d.PatternDitherStrategy(), d.ORDERED_STRATEGIES) and not isinstance(d.HalftoneDitherStrategy(), d.ORDERED_STRATEGIES)
    assert not hasattr(d.DitherMode, "PATTERN")                         # the enum stays the reference's


def test_image_ditherer_takes_a_strategy_instance():
    from dither_pie_amd import dithering_lib as d
    s = d.PatternDitherStrategy("8x8", 0.25)
    dith = d.ImageDitherer(num_colors=8, dither_mode=s, palette=[(0, 0, 0), (255, 255, 255)], dither_params={"ignored": 1})
    assert dith._get_dither_strategy(dith.dither_mode) is s
    h = d.HalftoneDitherStrategy(cell_size=4)
    assert d.ImageDitherer(dither_mode=h)._get_dither_strategy(h) is h
    back = pickle.loads(pickle.dumps(dith))
    assert isinstance(back.dither_mode, d.PatternDitherStrategy) and back.dither_mode.get_current_parameters() == s.get_current_parameters()
    assert back.palette == dith.palette and back.num_colors == 8
    # what the hook leaves alone
    with pytest.raises(NotImplementedError):
        d.ImageDitherer()._get_dither_strategy(d.DitherMode.HALFTONE)
    with pytest.raises(NotImplementedError):
        d.ImageDitherer()._get_dither_strategy(d.DitherMode.WAVELET)
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy("bayer")
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy(d.PatternDitherStrategy)   # the class is not an instance
    assert isinstance(d.ImageDitherer()._get_dither_strategy(d.DitherMode.BAYER), d.BayerDitherStrategy)


def test_backend_argument_errors_come_before_the_device():
    from dither_pie_amd import backend

    class P:
        K = 16
    for m in (3, "4x4", 0):
        with pytest.raises(ValueError, match="matrix"):
            backend.pattern(None, P(), m, 128)
    for s in (-1, 257, 0.5):
        with pytest.raises(ValueError, match="strength256"):
            backend.pattern(None, P(), 4, s)
    P.K = 257
    with pytest.raises(ValueError, match="256 colours"):
        backend.pattern(None, P(), 4, 128)
