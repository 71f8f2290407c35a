"""CPU tier of halftone dithering: the CPU restatement (tests/halftone_ref.py) against the reference's recorded outputs and
screens (tests/golden/halftone.*, from make_golden_halftone.py), the strategy's metadata and plumbing, and the argument
checks of the dp_halftone_* entry points (no GPU involved)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import halftone_ref


@pytest.fixture(scope="module")
def ht_json():
    with open(os.path.join(GOLDEN, "halftone.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ht_npz():
    return np.load(os.path.join(GOLDEN, "halftone.npz"))


@pytest.fixture(scope="module")
def lib():
    import dither_pie_amd
    if not os.path.exists(dither_pie_amd._lib.LIB_PATH):
        dither_pie_amd.build()
    return dither_pie_amd.load()


def ht_input(spec):
    from oracle import oracle as orc
    kind = spec[0]
    if kind == "rnd":
        return orc.rnd(spec[1], spec[2], spec[3])
    if kind == "grad":
        return orc.grad(spec[1], spec[2])
    if kind == "grey":
        return np.ascontiguousarray(orc.grad(spec[1], spec[2])[..., [0, 0, 0]])
    if kind == "imgl":
        return orc.imgl(spec[1], spec[2], spec[3])
    if kind == "tiegrey":
        y, x = np.mgrid[0:spec[1], 0:spec[2]]
        v = 5 + 10 * ((x // 24 + 3 * (y // 24)) % 25)
        return np.ascontiguousarray(np.stack([v, v, v], -1).astype(np.uint8))
    raise ValueError(spec)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _case_names():
    with open(os.path.join(GOLDEN, "halftone.json")) as fh:
        return [c["name"] for c in json.load(fh)["cases"]]


def test_inputs_are_the_recorded_ones(ht_json):
    for case in ht_json["cases"]:
        assert sha(ht_input(case["input"])) == case["input_sha256"], case["name"]


@pytest.mark.parametrize("name", _case_names())
def test_cpu_restatement_matches_reference(ht_json, ht_npz, name):
    case = next(c for c in ht_json["cases"] if c["name"] == name)
    arr = ht_input(case["input"])
    got = halftone_ref.apply(arr, [tuple(c) for c in case["palette"]], case["use_gamma"], **case["params"])
    if case.get("full"):
        assert np.array_equal(got, ht_npz["out_" + name])
    assert sha(got) == case["output_sha256"]


def test_cpu_restatement_matches_reference_screens(ht_json, ht_npz):
    for ent in ht_json["screens"]:
        scr, cells = halftone_ref.screen_with_cells(ent["h"], ent["w"], **dict(halftone_ref.DEFAULTS, **ent["params"]))
        assert str(scr.dtype) == ent["screen_dtype"] and str(cells.dtype) == ent["cells_dtype"]
        if ent.get("full"):
            assert np.array_equal(scr.view(np.uint32), ht_npz["screen_" + ent["name"]].view(np.uint32)), ent["name"]
            assert np.array_equal(cells, ht_npz["cells_" + ent["name"]]), ent["name"]
        assert sha(scr) == ent["screen_sha256"] and sha(cells) == ent["cells_sha256"], ent["name"]


def test_cpu_restatement_matches_reference_strategy(ht_json, ht_npz):
    for ent in ht_json["strategy"]:
        pal = ht_npz["st_pal_" + ent["name"]]
        arr = ht_input(ent["input"])
        got = pal[halftone_ref.halftone_idx(arr.astype(np.float32), pal, **ent["params"]).ravel()]
        assert np.array_equal(got, ht_npz["st_out_" + ent["name"]]) and sha(got) == ent["output_sha256"]


def test_host_fixup_thresholds_equal_the_full_screen(ht_json):
    """backend.halftone_thresholds_at (the host half of the pow class) reproduces the reference's screen pixel by pixel."""
    from dither_pie_amd import backend
    checked = 0
    for ent in ht_json["screens"]:
        p = dict(halftone_ref.DEFAULTS, **ent["params"])
        h, w = ent["h"], ent["w"]
        if h * w > 64 * 64:
            continue
        P = backend.halftone_params(np.zeros((1, 3), np.float32), **p)
        scr, _ = halftone_ref.screen_with_cells(h, w, **p)
        got = backend.halftone_thresholds_at(np.arange(h * w), w, P)
        if P.exp_class == backend.HT_EXP_POW:
            assert np.array_equal(got.view(np.uint32), scr.ravel().view(np.uint32)), ent["name"]
            checked += 1
    assert checked >= 2


def test_parameter_classes_and_paper():
    from dither_pie_amd import backend
    pal = np.array([[0, 0, 0], [250, 250, 250], [255, 255, 254], [255, 255, 254]], np.float32)
    for dg, cls in ((1.0, backend.HT_EXP_IDENTITY), (2.0, backend.HT_EXP_SQRT), (0.5, backend.HT_EXP_SQUARE),
                    (2, backend.HT_EXP_SQRT), (1.5, backend.HT_EXP_POW), (3.0, backend.HT_EXP_POW)):
        P = backend.halftone_params(pal, dot_gain=dg)
        assert P.exp_class == cls and P.exponent == 1.0 / dg
        assert P.paper_idx == 2 == halftone_ref.paper_index(pal)   # the first of two equally bright entries
    for shape, code in (("circle", 0), ("square", 1), ("diamond", 2), ("hexagon", 0)):
        assert backend.halftone_params(pal, shape=shape).shape == code
    P = backend.halftone_params(pal, angle=37.5)
    assert P.cos_a == np.cos(np.radians(37.5)) and P.sin_a == np.sin(np.radians(37.5))
    for bad in ({"cell_size": 0}, {"cell_size": -2}, {"cell_size": float("nan")}, {"dot_gain": 0.0}, {"dot_gain": -1.0},
                {"dot_gain": float("inf")}):
        with pytest.raises(ValueError):
            backend.halftone_params(pal, **bad)


def test_strategy_metadata_and_plumbing(kat):
    from dither_pie_amd import dithering_lib as d
    assert "HalftoneDitherStrategy" in d.__all__
    assert d.HalftoneDitherStrategy.get_parameter_info() == kat["misc"]["mode_parameters"]["halftone"]
    s = d.HalftoneDitherStrategy()
    assert isinstance(s, d.BaseDitherStrategy)
    assert s.get_current_parameters() == {k: v["default"] for k, v in kat["misc"]["mode_parameters"]["halftone"].items()}
    s2 = d.HalftoneDitherStrategy(cell_size=3, angle=10.0, dot_gain=2.0, min_dot_size=0.1, max_dot_size=0.9,
                                  shape="diamond", sharpness=1.0)
    assert s2.get_current_parameters() == dict(cell_size=3, angle=10.0, dot_gain=2.0, min_dot_size=0.1, max_dot_size=0.9,
                                               shape="diamond", sharpness=1.0)
    d.HalftoneDitherStrategy(cell_size=0, dot_gain=-1.0)   # the constructor validates nothing, as the reference's
    with pytest.raises(ValueError):   # a frame cannot be tiled: cells average over the whole image
        s._run(None, None, y0=4)
    with pytest.raises(ValueError):
        s._run(None, None, x0=1)
    with pytest.raises(ValueError):   # empty images are refused before anything touches the GPU
        s.dither(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.float32), (0, 5))


def test_image_ditherer_still_refuses_halftone():
    from dither_pie_amd import dithering_lib as d
    with pytest.raises(NotImplementedError):
        d.ImageDitherer()._get_dither_strategy(d.DitherMode.HALFTONE)
    assert d.ImageDitherer.get_mode_parameters(d.DitherMode.HALFTONE) is None
    assert d.DitherMode.HALFTONE not in d.ImageDitherer._STRATEGIES


def test_c_abi_argument_errors_without_gpu(lib):
    from dither_pie_amd import _lib, backend
    from dither_pie_amd._lib import DP_EINVAL, DP_EUNSUPPORTED, DP_OK
    for fn in ("dp_halftone_u8", "dp_halftone_workspace_bytes", "dp_halftone_pow_flags"):
        assert fn in _lib.EXPORTS and hasattr(lib, fn)
    assert lib.dp_version() == _lib.ABI_VERSION == 103
    fake = C.create_string_buffer(4096)   # a stand-in palette handle whose K field (the first int) is 4
    C.cast(fake, C.POINTER(C.c_int))[0] = 4
    pal = C.cast(fake, C.c_void_p)
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)

    def P(**kw):
        p = backend.halftone_params(np.zeros((4, 3), np.float32))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(p, n=1, h=2, w=2, pal_=pal, i=buf, o=buf, ws=buf):
        return lib.dp_halftone_u8(i, o, n, h, w, pal_, None if p is None else C.byref(p), ws, 1 << 20, None)

    assert call(P(), pal_=None) == DP_EINVAL and b"palette" in lib.dp_last_error()
    for n, h, w in ((-1, 2, 2), (1, -2, 2), (1, 2, -2)):
        assert call(P(), n, h, w) == DP_EINVAL and b"negative" in lib.dp_last_error()
    assert call(None) == DP_EINVAL and b"params" in lib.dp_last_error()
    for bad in (dict(cell_size=0.0), dict(cell_size=-8.0), dict(cell_size=float("inf"))):
        assert call(P(**bad)) == DP_EINVAL and b"cell_size" in lib.dp_last_error()
    for bad in (dict(cos_a=float("nan")), dict(exponent=float("inf")), dict(sharpness=float("nan")),
                dict(min_dot=float("-inf"))):
        assert call(P(**bad)) == DP_EINVAL and b"finite" in lib.dp_last_error()
    for bad in (dict(exp_class=4), dict(exp_class=-1), dict(shape=3)):
        assert call(P(**bad)) == DP_EINVAL and b"class or shape" in lib.dp_last_error()
    for bad in (dict(paper_idx=4), dict(paper_idx=-1)):
        assert call(P(**bad)) == DP_EINVAL and b"paper_idx" in lib.dp_last_error()
    for bad in (dict(reserved=1), dict(reserved=-7)):
        assert call(P(**bad)) == DP_EINVAL and b"reserved" in lib.dp_last_error()
    assert call(P(n_fix=3)) == DP_EINVAL and b"fix-up" in lib.dp_last_error()
    assert call(P(n_fix=-1)) == DP_EINVAL
    assert call(P(), i=None) == DP_EINVAL and b"NULL" in lib.dp_last_error()
    assert call(P(), o=None) == DP_EINVAL
    assert call(P(), ws=None) == DP_EINVAL and b"workspace" in lib.dp_last_error()
    # nothing to do: OK, buffers may be NULL
    assert call(P(), 0, 2, 2, i=None, o=None, ws=None) == DP_OK
    assert call(P(), 3, 0, 2, i=None, o=None, ws=None) == DP_OK
    # refused geometries (before any HIP call): too many cells, cells too large for uint32 sums
    assert call(P(cell_size=1e-6), 1, 4000, 4000) == DP_EUNSUPPORTED and b"cell" in lib.dp_last_error()
    assert call(P(cell_size=1e5), 1, 8000, 8000) == DP_EUNSUPPORTED and b"16843009" in lib.dp_last_error()
    # workspace size: cells of the default screen, 20 bytes each, plus the head; 0 for refused or bad arguments
    ws = lib.dp_halftone_workspace_bytes(24, 2160, 3840, C.byref(P()))
    assert 24 * 280000 * 20 < ws < 24 * 300000 * 20
    assert lib.dp_halftone_workspace_bytes(1, 4000, 4000, C.byref(P(cell_size=1e-6))) == 0
    assert lib.dp_halftone_workspace_bytes(1, 2, 2, None) == 0
    assert lib.dp_halftone_workspace_bytes(-1, 2, 2, C.byref(P())) == 0
    assert lib.dp_halftone_pow_flags(2, 2, C.byref(P()), buf, 4, None, None) == DP_EINVAL
    assert lib.dp_halftone_pow_flags(-2, 2, C.byref(P()), buf, 4, buf, None) == DP_EINVAL
    assert lib.dp_halftone_pow_flags(2, 2, C.byref(P(cell_size=0.0)), buf, 4, buf, None) == DP_EINVAL
    assert lib.dp_halftone_pow_flags(2, 2, None, buf, 4, buf, None) == DP_EINVAL
