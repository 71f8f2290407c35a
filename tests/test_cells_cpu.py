"""CPU tier of cell-palette dithering (include/ditherpie_hip_cells.h, dithering_lib.CellPaletteDitherStrategy): the agreement
of the header, the ctypes table, the exported symbols and the memory-discipline module (the rule tests/test_dotdiff_cpu.py
keeps for its header); dp_cells_candidates (host code) against the enumeration of tests/cells_ref.py; properties of the numpy
statement that follow from the definition alone; the refusals of dp_cells_u8, which happen before any HIP call; the Python
surface.  The rank-to-mask function of host_logic.h has no host export: it is held to the statement through the `sets`
output of the GPU tier (tests/test_gpu_cells.py)."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import cells_ref as cr
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_cells.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_cells_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_cells_candidates", "dp_cells_u8"} == set(_lib.EXPORTS_CELLS)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP) | set(_lib.EXPORTS_SCENE) | set(_lib.EXPORTS_GIF)
              | set(_lib.EXPORTS_PNG) | set(_lib.EXPORTS_PNG_DYN) | set(_lib.EXPORTS_PATTERN) | set(_lib.EXPORTS_PNG_FILE)
              | set(_lib.EXPORTS_DOTDIFF))
    assert not set(_lib.EXPORTS_CELLS) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_CELLS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    with_dev = {n for n, a in found.items() if re.search(r"\w+_dev\b", a)}   # the device entry points: whatever takes a *_dev pointer
    assert with_dev == {"dp_cells_u8"}
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
    for name in _lib.EXPORTS_CELLS:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: cells.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_CELLS:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    assert backend.CELL_SIZES == cr.CELL_SIZES == (4, 8, 16) and backend.CELL_MATRICES == cr.MATRICES == (2, 4, 8)


# ---------------------------------------------------------------------------------------------------- the candidate count
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _count(lib, K, k, fixed, groups):
    g = np.array(list(groups), np.uint16)
    return lib.dp_cells_candidates(K, k, fixed, g.ctypes.data if len(g) else None, len(g))


def _groups_for(K, n, rs):
    """n overlapping groups of a palette of K entries: the whole palette, its lower and upper part (sharing the middle) and a
    random non-empty mask."""
    full = (1 << K) - 1
    lo = full & ((1 << (K // 2 + 1)) - 1)
    hi = full & ~((1 << (K // 2)) - 1)
    rnd = int(rs.randint(1, full + 1))
    return [full, lo, hi, rnd][:n]


def test_candidate_count_equals_the_enumeration(lib):
    rs = np.random.RandomState(404)
    seen_valid = seen_invalid = 0
    for K in range(1, 17):
        for k in range(1, 5):
            for fixed in (0, 1, (1 << K) >> 1 | 1, int(rs.randint(0, 1 << K))):
                for n in range(1, 5):
                    groups = _groups_for(K, n, rs)
                    try:
                        want = len(cr.candidates(K, k, fixed, groups))
                        seen_valid += 1
                    except ValueError:
                        want = -1
                        seen_invalid += 1
                    assert _count(lib, K, k, fixed, groups) == want, (K, k, fixed, groups)
    assert seen_valid > 300 and seen_invalid > 100                      # both sides occur
    assert _count(lib, 16, 4, 0, [0xFFFF] * 4) == 7280 == 4 * 1820
    assert _count(lib, 15, 2, 0, [0x00FF, 0x7F01]) == 56 == len(cr.candidates(15, 2, 0, [0x00FF, 0x7F01]))   # the ZX pair
    assert _count(lib, 16, 3, 1, [0xFFFF]) == 455                       # C64 multicolour: three of the fifteen others


def test_candidate_count_refuses_every_invalid_combination(lib):
    ok = dict(K=16, k=2, fixed=0, groups=[0xFFFF])
    assert _count(lib, **ok) == 120
    for bad in (dict(K=0), dict(K=-1), dict(K=17), dict(K=256), dict(k=0), dict(k=5), dict(k=-1), dict(groups=[]),
                dict(groups=[0xFFFF] * 5), dict(groups=[0]), dict(groups=[0xFFFF, 0]), dict(K=15, groups=[0xFFFF]),
                dict(K=15, fixed=0x8000, groups=[0x7FFF]), dict(K=4, fixed=0x10, groups=[0xF]), dict(fixed=0x10000),
                dict(k=3, groups=[0x3]), dict(k=2, fixed=0x1, groups=[0x3]), dict(k=2, fixed=0xFFFE), dict(K=1, k=2, groups=[1])):
        assert _count(lib, **dict(ok, **bad)) == -1, bad
    assert lib.dp_cells_candidates(16, 2, 0, None, 1) == -1
    assert _count(lib, 1, 1, 0, [1]) == 1 and _count(lib, 2, 1, 1, [3]) == 1 and _count(lib, 2, 1, 1, [2]) == 1


def test_enumeration_order_of_the_statement():
    assert cr.candidates(4, 2, 0, [0xF]) == [0b0011, 0b0101, 0b1001, 0b0110, 0b1010, 0b1100]
    assert cr.candidates(4, 1, 0b0001, [0b0111, 0b1100]) == [0b0011, 0b0101, 0b0101, 0b1001]   # overlapping groups repeat a set
    assert cr.candidates(5, 2, 0b00100, [0b11111])[:3] == [0b00111, 0b01101, 0b10101]
    zx = cr.candidates(15, 2, 0, [0x00FF, 0x7F01])
    assert len(zx) == 56 and zx[0] == 0b11 and zx[28] == 0x0101 and zx[-1] == 0x6000


# ---------------------------------------------------------------------------------------------------- the statement
def _pal(rs, K):
    pal = rs.randint(0, 256, (K, 3)).astype(np.float32)
    return pal, pal.astype(np.uint8)


def test_every_cell_uses_colours_of_its_set_only():
    rs = np.random.RandomState(11)
    pal, outc = _pal(rs, 8)
    outc = np.arange(24, dtype=np.uint8).reshape(8, 3)                  # distinct bytes: an output pixel names its entry
    img = rs.randint(0, 256, (21, 27, 3)).astype(np.uint8)
    for cw, ch, k, fixed, groups in ((8, 8, 2, 0, [0xFF]), (4, 8, 3, 0b1, [0xFF]), (16, 4, 1, 0b11, [0x3C, 0xF0]), (4, 4, 4, 0, [0x0F, 0xFF])):
        out, sets = cr.cells_u8(img, pal, outc, None, cw, ch, k, fixed, groups, 4, 64)
        cand = set(cr.candidates(8, k, fixed, groups))
        assert sets.shape == (-(-21 // ch), -(-27 // cw))
        for cy in range(sets.shape[0]):
            for cx in range(sets.shape[1]):
                S = int(sets[cy, cx])
                assert S in cand and S & fixed == fixed and bin(S).count("1") == k + bin(fixed).count("1")
                used = {int(v) // 3 for v in out[cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw, 0].reshape(-1)}
                assert used <= set(cr.bits_of(S)) and len(used) <= bin(S).count("1")


def test_whole_palette_without_spread_is_a_nearest_colour():
    rs = np.random.RandomState(12)
    pal, outc = _pal(rs, 4)
    lut = rs.permutation(256).astype(np.uint8)
    img = rs.randint(0, 256, (9, 13, 3)).astype(np.uint8)
    for lut_in in (None, lut):
        idx, sets = cr.cells_indices(img, pal, lut_in, 4, 8, 4, 0, [0xF], 8, 0)
        assert (sets == 0xF).all()
        c = (lut_in[img] if lut_in is not None else img).astype(np.int64)
        d = ((c[:, :, None, :] - np.trunc(pal).astype(np.int64)[None, None]) ** 2).sum(-1)
        assert np.array_equal(np.take_along_axis(d, idx[:, :, None], -1)[:, :, 0], d.min(-1))
        assert np.array_equal(idx, d.argmin(-1))                        # ... and the lowest index among equals


def test_flat_palette_colour_takes_the_first_candidate_that_holds_it():
    rs = np.random.RandomState(13)
    pal, outc = _pal(rs, 6)
    groups = [0b000111, 0b111100, 0b111111]
    for k, fixed in ((2, 0), (1, 0b100), (3, 0)):
        cand = cr.candidates(6, k, fixed, groups)
        for j in range(6):
            img = np.broadcast_to(outc[j], (9, 10, 3)).copy()
            out, sets = cr.cells_u8(img, pal, outc, None, 8, 4, k, fixed, groups, 4, 0)
            first = next(s for s in cand if (s >> j) & 1)
            assert (sets == first).all() and np.array_equal(out, img), (k, fixed, j)


def test_grey_ramp_white_count_rises_by_two():
    """8 x 8 cells, {black, white}, m = 8, spread 255: cell i of a ramp of 32 grey levels shows 2 i white pixels -- the
    perturbation, not the cell's mean, decides the pattern."""
    bw = np.array([[0, 0, 0], [255, 255, 255]], np.float32)
    levels = [8 * i for i in range(32)]
    img = np.repeat(np.array(levels, np.uint8), 8)[None, :, None] * np.ones((8, 1, 3), np.uint8)
    idx, sets = cr.cells_indices(img, bw, None, 8, 8, 2, 0, [0b11], 8, 255)
    white = idx.reshape(8, 32, 8).sum(axis=(0, 2))
    print("white pixels per cell:", white.tolist())
    assert white.tolist() == list(range(0, 64, 2)) and (sets == 0b11).all()


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


def test_cells_refusals(lib):
    fn = "dp_cells_u8"
    keep = _fake_palette(16)
    g1 = np.array([0xFFFF], np.uint16)
    ok = dict(i=0x1001, o=0x2000003, s=0x3000002, n=3, h=4, w=5, pal=C.cast(keep, C.c_void_p), cw=8, ch=8, k=2, fixed=0,
              g=g1.ctypes.data, ng=1, m=4, spread=64)                   # never dereferenced

    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_cells_u8(v["i"], v["o"], v["s"], v["n"], v["h"], v["w"], v["pal"], v["cw"], v["ch"], v["k"], v["fixed"], v["g"],
                               v["ng"], v["m"], v["spread"], None)

    for bad in (dict(i=None), dict(o=None), dict(pal=None), dict(g=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-7), dict(n=-1),
                dict(h=65536, w=65536)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for bad in (dict(cw=0), dict(cw=2), dict(cw=12), dict(cw=32), dict(ch=1), dict(ch=-8), dict(ch=64)):
        _refused(lib, call(**bad), 1, fn, "cell")
    for m in (0, 1, 3, 16, -2):
        _refused(lib, call(m=m), 1, fn, "matrix")
    for s in (-1, 256, 1000):
        _refused(lib, call(spread=s), 1, fn, "spread")
    for bad in (dict(k=0), dict(k=5), dict(k=-1), dict(ng=0), dict(ng=5), dict(ng=-1)):
        _refused(lib, call(**bad), 1, fn, "1 .. 4")
    _refused(lib, call(s=0x3000001), 1, fn, "sets_dev")
    empty, small, two = np.array([0], np.uint16), np.array([0x0003], np.uint16), np.array([0xFFFF, 0x8000], np.uint16)
    for bad in (dict(g=empty.ctypes.data), dict(g=small.ctypes.data, k=3), dict(g=small.ctypes.data, fixed=1), dict(fixed=0x10000),
                dict(g=two.ctypes.data, ng=2, k=2)):
        _refused(lib, call(**bad), 1, fn, "groups")
    five = _fake_palette(5)
    _refused(lib, call(pal=C.cast(five, C.c_void_p)), 1, fn, "below 5")  # a group bit at or above K
    _refused(lib, call(pal=C.cast(five, C.c_void_p), g=np.array([0x1F], np.uint16).ctypes.data, fixed=0x20), 1, fn, "below 5")
    for n in (3, 0):                                                    # the palette is checked before "nothing to do"
        big = _fake_palette(17)
        _refused(lib, call(pal=C.cast(big, C.c_void_p), n=n), 2, fn, "16")   # DP_EUNSUPPORTED
    assert call(n=0) == 0 and call(n=0, i=None, o=None, s=None) == 0    # nothing to do is not an error, and launches nothing
    _refused(lib, call(n=0, m=3), 1, fn, "matrix")                      # ... but a bad argument still is one


# ---------------------------------------------------------------------------------------------------- Python surface
def test_strategy_metadata_and_parameters():
    from dither_pie_amd import dithering_lib as d
    S = d.CellPaletteDitherStrategy
    assert "CellPaletteDitherStrategy" in d.__all__ and issubclass(S, d.BaseDitherStrategy)
    info = S.get_parameter_info()
    assert list(info) == ["cell", "colours", "matrix", "spread"]
    assert info["cell"]["default"] == "8x8" and "4x8" in info["cell"]["choices"] and len(info["cell"]["choices"]) == 9
    assert (info["colours"]["min"], info["colours"]["max"], info["colours"]["default"]) == (1, 4, 2)
    assert info["matrix"]["choices"] == ["2x2", "4x4", "8x8"] and info["matrix"]["default"] == "4x4"
    assert (info["spread"]["min"], info["spread"]["max"], info["spread"]["default"]) == (0, 255, 64)
    s = S()
    assert s.get_current_parameters() == {"cell": "8x8", "colours": 2, "matrix": "4x4", "spread": 64, "shared": (), "groups": None}
    assert s._settings() == ((8, 8), 2, 4, 64, 0, None)
    assert S(cell="4x8", colours=3, shared=(0,))._settings() == ((4, 8), 3, 4, 64, 1, None)          # C64 multicolour
    assert S(cell=(16, 4), colours=1, matrix=8, spread=0, shared=[1, 3], groups=[[0, 2], range(4, 8)])._settings() == \
        ((16, 4), 1, 8, 0, 0b1010, [0b0101, 0xF0])
    for bad in (dict(cell="8"), dict(cell="8x"), dict(cell="8x8x8"), dict(cell="5x8"), dict(cell="axb"), dict(cell=(8,)), dict(cell=8),
                dict(cell=(8, 32)), dict(colours=0), dict(colours=5), dict(colours=2.0), dict(matrix="3x3"), dict(matrix=16),
                dict(spread=-1), dict(spread=256), dict(spread=1.5), dict(shared=(16,)), dict(shared=(-1,)), dict(shared=3),
                dict(groups=[[0, 16]]), dict(groups=[3]), dict(groups=7)):
        with pytest.raises(ValueError):
            S(**bad)._settings()
    assert not isinstance(s, d.ORDERED_STRATEGIES)                      # a band edge would split cells
    assert not hasattr(d.DitherMode, "CELL_PALETTE") and len(d.DitherMode) == len({m.value for m in d.DitherMode})
    with pytest.raises(ValueError, match="non-empty"):
        s.dither(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.float32), (0, 5))
    with pytest.raises(ValueError, match="16 colours"):
        s.dither(np.zeros((4, 3), np.float32), np.zeros((17, 3), np.float32), (2, 2))
    with pytest.raises(ValueError, match="below 2"):                    # an index at or above K
        S(shared=(2,)).dither(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), (2, 2))
    with pytest.raises(ValueError, match="fewer than 3"):               # a group too small
        S(colours=3).dither(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), (2, 2))

    class P:
        K = 16
    for kw in (dict(y0=8), dict(x0=4)):
        with pytest.raises(ValueError, match="tiled"):
            s._run(None, P(), **kw)
    P.K = 17
    with pytest.raises(ValueError, match="16 colours"):
        s._run(None, P())


def test_zx_spectrum_preset():
    from dither_pie_amd import dithering_lib as d
    S = d.CellPaletteDitherStrategy
    pal = S.ZX_SPECTRUM_PALETTE
    assert len(pal) == 15 and pal[0] == (0, 0, 0)
    assert pal[1:8] == [(0, 0, 215), (215, 0, 0), (215, 0, 215), (0, 215, 0), (0, 215, 215), (215, 215, 0), (215, 215, 215)]
    assert pal[8:] == [tuple(255 if v else 0 for v in c) for c in pal[1:8]] and len(set(pal)) == 15
    zx = S.zx_spectrum()
    assert zx._settings() == ((8, 8), 2, 4, 64, 0, [0x00FF, 0x7F01])
    assert S.zx_spectrum(matrix="8x8", spread=200)._settings() == ((8, 8), 2, 8, 200, 0, [0x00FF, 0x7F01])
    from dither_pie_amd import backend
    assert backend.cell_candidates(15, 2, 0, [0x00FF, 0x7F01]) == 56


def test_image_ditherer_takes_the_instance():
    from dither_pie_amd import dithering_lib as d
    s = d.CellPaletteDitherStrategy.zx_spectrum(spread=32)
    dith = d.ImageDitherer(num_colors=15, dither_mode=s, palette=d.CellPaletteDitherStrategy.ZX_SPECTRUM_PALETTE, dither_params={"ignored": 1})
    assert dith._get_dither_strategy(dith.dither_mode) is s
    back = pickle.loads(pickle.dumps(dith))
    assert isinstance(back.dither_mode, d.CellPaletteDitherStrategy) and back.dither_mode.spread == 32
    assert back.dither_mode._settings() == s._settings() and back.palette == dith.palette
    with pytest.raises(ValueError):
        d.ImageDitherer()._get_dither_strategy(d.CellPaletteDitherStrategy)   # the class is not an instance


def test_backend_argument_errors_come_before_the_device():
    from dither_pie_amd import backend

    class P:
        K = 16
    ok = dict(cell=(8, 8), colours=2, matrix=4, spread=64)

    def call(**kw):
        v = dict(ok, **kw)
        return backend.cells(None, P(), v.pop("cell"), v.pop("colours"), v.pop("matrix"), v.pop("spread"), **v)

    for cell in ("8x8", 8, (8,), (8, 5), (32, 8), (8, 8, 8), None):
        with pytest.raises(ValueError, match="cell must"):
            call(cell=cell)
    for k in (0, 5, -1, 2.0, None):
        with pytest.raises(ValueError, match="1 .. 4"):
            call(colours=k)
    for m in (0, 3, 16, "4x4"):
        with pytest.raises(ValueError, match="matrix"):
            call(matrix=m)
    for s in (-1, 256, 0.5):
        with pytest.raises(ValueError, match="spread"):
            call(spread=s)
    for fixed in (-1, 1 << 16, 0.5):
        with pytest.raises(ValueError, match="fixed_mask"):
            call(fixed_mask=fixed)
    for groups in ([], [1] * 5, 7):
        with pytest.raises(ValueError, match="groups"):
            call(groups=groups)
    for groups in ([0], [1 << 16], [0xFFFF, 0.5]):
        with pytest.raises(ValueError, match="group"):
            call(groups=groups)
    with pytest.raises(ValueError, match="fewer than 3"):
        call(colours=3, groups=[0b11])
    with pytest.raises(ValueError, match="fewer than 2"):
        call(fixed_mask=0b1, groups=[0b11])
    P.K = 5
    with pytest.raises(ValueError, match="below 5"):
        call(groups=[0b100000])
    with pytest.raises(ValueError, match="below 5"):
        call(fixed_mask=0b100000)
    P.K = 17
    with pytest.raises(ValueError, match="16 colours"):
        call()
    assert backend.cell_candidates(16, 4) == 1820 and backend.cell_candidates(16, 2, 0, [0xFFFF] * 4) == 480
    assert backend.cell_candidates(16, 3, 1) == 455
    for bad in (dict(K=0, colours=1), dict(K=17, colours=1), dict(K=4, colours=5), dict(K=4, colours=2, groups=[0b1]),
                dict(K=4, colours=1, groups=[0b10000]), dict(K=4, colours=1, fixed_mask=0b10000)):
        with pytest.raises(ValueError):
            backend.cell_candidates(**bad)
