"""CPU tier of wavelet dithering: the CPU restatement (tests/wavelet_ref.py) against the reference's recorded outputs,
reconstructions and subbands (tests/golden/wavelet.*, from make_golden_wavelet.py), the k=2 stage under this scipy against
the recording one, the strategy's metadata and plumbing, and the argument checks of the dp_wavelet_* entry points (no GPU
involved)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import wavelet_ref as wr


@pytest.fixture(scope="module")
def wl_json():
    with open(os.path.join(GOLDEN, "wavelet.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def wl_npz():
    return np.load(os.path.join(GOLDEN, "wavelet.npz"))


@pytest.fixture(scope="module")
def lib():
    import dither_pie_amd
    if not os.path.exists(dither_pie_amd._lib.LIB_PATH):
        dither_pie_amd.build()
    return dither_pie_amd.load()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _cases(max_px=None):
    with open(os.path.join(GOLDEN, "wavelet.json")) as fh:
        cases = json.load(fh)["cases"]
    return [c["name"] for c in cases if max_px is None or c["h"] * c["w"] <= max_px]


def _case(js, name):
    return next(c for c in js["cases"] if c["name"] == name)


def test_fixture_coverage(wl_json):
    cases = wl_json["cases"]
    assert {c["params"].get("wavelet", "haar") for c in cases} == set(wr.WAVELETS)
    assert {1, 2, 8, 32, 33, 70000} <= {c["params"].get("subband_quant", 8) for c in cases}
    assert {0, 42, 9999} <= {c["params"].get("seed", 42) for c in cases}
    assert any(c["params"].get("seed", 42) > 9999 for c in cases)
    assert any(c["use_gamma"] for c in cases) and any(not c["use_gamma"] for c in cases)
    assert {2, 1024} <= {len(c["palette"]) for c in cases}
    assert any(c["h"] == 2160 and c["w"] == 3840 for c in cases)
    assert sum(c["h"] == 1080 and c["w"] == 1920 for c in cases) == 3


def test_inputs_are_the_recorded_ones(wl_json):
    for case in wl_json["cases"]:
        assert sha(wr.make_input(case["input"])) == case["input_sha256"], case["name"]


def test_taps_are_the_libraries(wl_json):
    """The fixture's impulse taps are the filters compiled into wavelet.hip (read back from its source)."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "dither_pie_amd", "csrc", "wavelet.hip")).read()
    body = src[src.index("c_taps[9][4][kMaxF] = {"):]
    body = body[:body.index("};")]
    import re
    vals = [float.fromhex(t[:-1]) if "x" in t else float(t[:-1]) for t in re.findall(r"-?0x[0-9a-f.]+p[-+]\d+f|-?0\.0f", body)]
    pos = 0
    for wname in wr.WAVELETS:
        T = wl_json["taps"][wname]
        for key in ("dec_lo", "dec_hi", "rec_lo", "rec_hi"):
            F = len(T[key])
            assert vals[pos:pos + F] == T[key], (wname, key)
            assert np.float32(T[key]).tolist() == T[key]
            pos += F
    assert pos == len(vals)
    # filter lengths 2, 4, 6 and 8 all occur
    assert len({len(wl_json["taps"][w]["dec_lo"]) for w in wr.WAVELETS}) == 4


def test_dec_terms_cover_each_output_once():
    for F in (2, 4, 6, 8):
        for N in range(1, 20):
            for t in wr.dec_terms(N, F):
                assert sorted(m for m, _ in t) == list(range(F))
                assert all(0 <= k < N for _, k in t)


@pytest.mark.parametrize("name", _cases(300 * 300))
def test_cpu_restatement_matches_reference(wl_json, wl_npz, name):
    case = _case(wl_json, name)
    arr = wr.make_input(case["input"])
    got = wr.apply(arr, [tuple(c) for c in case["palette"]], case["use_gamma"], wl_json["taps"], **case["params"])
    if case.get("full"):
        assert np.array_equal(got, wl_npz["out_" + name])
    assert sha(got) == case["output_sha256"]


@pytest.mark.parametrize("name", _cases(2500))
def test_cpu_restatement_intermediates(wl_json, wl_npz, name):
    """the float32 reconstructions (the k=2 query points) and, where stored, the float32 subbands, bit for bit"""
    from oracle import oracle as orc
    case = _case(wl_json, name)
    assert case["rec"]
    p = dict(case["params"])
    T = wr.taps_of(wl_json["taps"], p.get("wavelet", "haar"))
    _, _, lut_in = orc.prepare_palette([tuple(c) for c in case["palette"]], case["use_gamma"])
    arr = wr.make_input(case["input"])
    src = (arr if lut_in is None else np.asarray(lut_in)[arr]).astype(np.float32)
    h, w = case["h"], case["w"]
    u = wr.uniforms(p.get("seed", 42), h, w, len(T["dec_lo"]))
    rec, _, subs = wr.reconstruct(src, T, p.get("subband_quant", 8), u)
    assert np.array_equal(rec.view(np.uint32), wl_npz["rec_" + name].view(np.uint32))
    assert sha(rec.reshape(-1, 3)) == case["points_sha256"]
    if case.get("subbands"):
        for ch in range(3):
            for s, sb in zip("AHVD", subs[ch]):
                ref = wl_npz[f"sb_{name}_{ch}{s}"]
                assert sb.shape == ref.shape and np.array_equal(sb.view(np.uint32), ref.view(np.uint32)), (ch, s)


def test_k2_stage_under_this_scipy(wl_json, wl_npz):
    """The fixtures come from scipy 1.7.1; this interpreter's scipy (KDTree.query(k=2) on the recorded float32
    reconstructions, ties included) must pick the same entries: every stored reconstruction, re-picked here, gives the
    recorded output."""
    from oracle import oracle as orc
    assert wl_json["versions"]["scipy"] == "1.7.1"
    n = 0
    for case in wl_json["cases"]:
        if not (case.get("rec") and case.get("full")):
            continue
        p = case["params"]
        F = len(wl_json["taps"][p.get("wavelet", "haar")]["dec_lo"])
        h, w = case["h"], case["w"]
        pal_f32, out_colors, lut_in = orc.prepare_palette([tuple(c) for c in case["palette"]], case["use_gamma"])
        u = wr.uniforms(p.get("seed", 42), h, w, F)
        rec = wl_npz["rec_" + case["name"]]
        # the thresholds follow the subband draws: their count from the restatement (whose subbands and reconstructions
        # are pinned above)
        arr = wr.make_input(case["input"])
        src = (arr if lut_in is None else np.asarray(lut_in)[arr]).astype(np.float32)
        _, pos, _ = wr.reconstruct(src, wr.taps_of(wl_json["taps"], p.get("wavelet", "haar")), p.get("subband_quant", 8), u)
        idx = wr.pick(rec, pal_f32, u[pos:pos + h * w])
        assert np.array_equal(out_colors[idx].reshape(h, w, 3), wl_npz["out_" + case["name"]]), case["name"]
        n += 1
    assert n >= 25


def test_cpu_restatement_matches_reference_strategy(wl_json, wl_npz):
    for ent in wl_json["strategy"]:
        pal = wl_npz["st_pal_" + ent["name"]]
        arr = wr.make_input(ent["input"])
        got = pal[wr.dither_indices(arr.astype(np.float32), pal, wl_json["taps"], **ent["params"])]
        assert np.array_equal(got, wl_npz["st_out_" + ent["name"]]) and sha(got) == ent["output_sha256"]


def test_strategy_metadata_and_plumbing(kat):
    from dither_pie_amd import dithering_lib as d
    assert "WaveletDitherStrategy" in d.__all__
    assert d.WaveletDitherStrategy.get_parameter_info() == kat["misc"]["mode_parameters"]["wavelet"]
    s = d.WaveletDitherStrategy()
    assert isinstance(s, d.BaseDitherStrategy)
    assert s.get_current_parameters() == {k: v["default"] for k, v in kat["misc"]["mode_parameters"]["wavelet"].items()}
    s2 = d.WaveletDitherStrategy(wavelet="db4", subband_quant=3, seed=7)
    assert s2.get_current_parameters() == dict(wavelet="db4", subband_quant=3, seed=7)
    d.WaveletDitherStrategy(wavelet="mexh", subband_quant=0, seed=-1)   # the constructor validates nothing
    with pytest.raises(ValueError):   # a frame cannot be tiled: the subband extremes span the image
        s._run(None, None, y0=4)
    with pytest.raises(ValueError):
        s._run(None, None, x0=1)
    with pytest.raises(ValueError):   # empty images are refused before anything touches the GPU
        s.dither(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.float32), (0, 5))


def test_divergences_raise_value_error():
    from dither_pie_amd import backend
    from dither_pie_amd import dithering_lib as d
    assert backend.wavelet_check() == (0, 8, 42)
    assert backend.wavelet_check("bior2.2", 1, 0) == (8, 1, 0)
    assert backend.wavelet_check("sym4", 2 ** 31 - 1, 2 ** 32 - 1) == (5, 2 ** 31 - 1, 2 ** 32 - 1)
    assert backend.wavelet_check("db2", np.int64(33), np.uint32(5)) == (2, 33, 5)
    bad = [dict(wavelet="db3"), dict(wavelet="mexh"), dict(wavelet=None), dict(subband_quant=0), dict(subband_quant=-2),
           dict(subband_quant=2.0), dict(subband_quant=True), dict(subband_quant=2 ** 31), dict(seed=-1),
           dict(seed=2 ** 32), dict(seed=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            backend.wavelet_check(**kw)
        with pytest.raises(ValueError):   # at dither time, before anything touches the GPU
            d.WaveletDitherStrategy(**kw).dither(np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), (2, 2))


def test_image_ditherer_still_refuses_wavelet():
    from dither_pie_amd import dithering_lib as d
    with pytest.raises(NotImplementedError):
        d.ImageDitherer()._get_dither_strategy(d.DitherMode.WAVELET)
    assert d.ImageDitherer.get_mode_parameters(d.DitherMode.WAVELET) is None
    assert d.DitherMode.WAVELET not in d.ImageDitherer._STRATEGIES


class _Params(C.Structure):
    _fields_ = [("wavelet", C.c_int32), ("subband_quant", C.c_int32), ("uniforms_dev", C.c_void_p),
                ("n_uniforms", C.c_int64)]


def test_c_abi_argument_errors_without_gpu(lib):
    from dither_pie_amd import _lib, backend
    from dither_pie_amd._lib import DP_EINVAL, DP_EUNSUPPORTED, DP_OK
    for fn in ("dp_wavelet_u8", "dp_wavelet_workspace_bytes", "dp_wavelet_uniforms_needed"):
        assert fn in _lib.EXPORTS and hasattr(lib, fn)
    assert lib.dp_version() == _lib.ABI_VERSION == 103
    assert [f[0] for f in backend.WaveletParams._fields_] == [f[0] for f in _Params._fields_]
    fake = C.create_string_buffer(4096)   # a stand-in palette handle whose K field (the first int) is 4
    C.cast(fake, C.POINTER(C.c_int))[0] = 4
    pal = C.cast(fake, C.c_void_p)
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    # stream length: 12 subbands of ((h + F - 1) // 2) x ((w + F - 1) // 2), then h * w
    for wid, F in enumerate((2, 2, 4, 8, 4, 8, 6, 6, 6)):
        for h, w in ((1, 1), (3, 5), (1080, 1920), (2160, 3840)):
            assert lib.dp_wavelet_uniforms_needed(h, w, wid) == 12 * ((h + F - 1) // 2) * ((w + F - 1) // 2) + h * w
    assert lib.dp_wavelet_uniforms_needed(4, 4, 9) == -1 and lib.dp_wavelet_uniforms_needed(-1, 4, 0) == -1
    assert lib.dp_wavelet_uniforms_needed(0, 4, 0) == 0
    need = lib.dp_wavelet_uniforms_needed(2, 2, 0)

    def P(wavelet=0, q=8, u=buf, n=need):
        return _Params(wavelet, q, u, n)

    def call(p, n=1, h=2, w=2, pal_=pal, i=buf, o=buf, ws=buf):
        return lib.dp_wavelet_u8(i, o, n, h, w, pal_, None if p is None else C.byref(p), ws, 1 << 20, None)

    assert call(P(), pal_=None) == DP_EINVAL and b"palette" in lib.dp_last_error()
    for n, h, w in ((-1, 2, 2), (1, -2, 2), (1, 2, -2)):
        assert call(P(), n, h, w) == DP_EINVAL and b"negative" in lib.dp_last_error()
    assert call(None) == DP_EINVAL and b"params" in lib.dp_last_error()
    for wid in (-1, 9, 100):
        assert call(P(wavelet=wid)) == DP_EINVAL and b"wavelet" in lib.dp_last_error()
    for q in (0, -1):
        assert call(P(q=q)) == DP_EINVAL and b"subband_quant" in lib.dp_last_error()
    assert call(P(n=need - 1)) == DP_EINVAL and b"stream" in lib.dp_last_error()
    assert call(P(u=None)) == DP_EINVAL and b"stream" in lib.dp_last_error()
    assert call(P(), i=None) == DP_EINVAL and b"NULL" in lib.dp_last_error()
    assert call(P(), o=None) == DP_EINVAL
    assert call(P(), ws=None) == DP_EINVAL and b"workspace" in lib.dp_last_error()
    assert call(P(), 0, 2, 2, i=None, o=None, ws=None) == DP_OK
    assert call(P(), 3, 0, 2, i=None, o=None, ws=None) == DP_OK
    assert call(P(n=1 << 40), 1, 50000, 50000) == DP_EUNSUPPORTED
    # workspace: a head, six planes of n0 x w, 12 subbands, a word per pixel; frames in groups of <= 512 MB
    h, w = 1080, 1920
    per = 256 + 4 * (6 * 540 * w + 12 * 540 * 960 + h * w)
    assert lib.dp_wavelet_workspace_bytes(1, h, w, C.byref(P())) == per
    assert lib.dp_wavelet_workspace_bytes(100, h, w, C.byref(P())) == ((512 << 20) // per) * per
    assert lib.dp_wavelet_workspace_bytes(24, 2160, 3840, C.byref(P())) >= 1
    assert lib.dp_wavelet_workspace_bytes(1, 2, 2, None) == 0
    assert lib.dp_wavelet_workspace_bytes(1, 2, 2, C.byref(P(wavelet=9))) == 0
    assert lib.dp_wavelet_workspace_bytes(-1, 2, 2, C.byref(P())) == 0
