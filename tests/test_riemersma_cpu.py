"""CPU tier of the Riemersma mode: the drop-in's path helpers and the CPU restatement (tests/riemersma_ref.py) against the
reference's recorded outputs (tests/golden/riemersma.*, from make_golden_riemersma.py), the strategy plumbing, and the
argument checks of dp_riemersma_u8 (no GPU involved)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import riemersma_ref


@pytest.fixture(scope="module")
def rm_json():
    with open(os.path.join(GOLDEN, "riemersma.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def rm_npz():
    return np.load(os.path.join(GOLDEN, "riemersma.npz"))


@pytest.fixture(scope="module")
def lib():
    import dither_pie_amd
    if not os.path.exists(dither_pie_amd._lib.LIB_PATH):
        dither_pie_amd.build()
    return dither_pie_amd.load()


def rm_input(spec):
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
    raise ValueError(spec)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_hilbert_order_and_next_power_of_two_mirror_the_reference(rm_json, rm_npz):
    from dither_pie_amd import dithering_lib as d
    for k in range(7):
        n = 1 << k
        got = d._hilbert_order(n)
        assert got.dtype == np.int32 and got.shape == (n * n, 2)
        assert np.array_equal(got, rm_npz[f"hilbert_{n}"]), n
        assert sha(got) == rm_json["hilbert"][str(n)]
        r, c = riemersma_ref.path_rc(n)
        assert np.array_equal(np.stack([r, c], 1), got)
    xs, want = rm_npz["npot_x"], rm_npz["npot"]
    assert [d._next_power_of_two(int(x)) for x in xs] == [int(v) for v in want]


def test_inputs_are_the_recorded_ones(rm_json):
    for case in rm_json["cases"]:
        if case["h"] * case["w"] <= 300 * 300:
            assert sha(rm_input(case["input"])) == case["input_sha256"], case["name"]


@pytest.mark.parametrize("name", ["rm_1x1_p2", "rm_1x300_p8", "rm_300x1_p16_g", "rm_37x53_p2", "rm_37x53_p17",
                                  "rm_37x53_p17_g", "rm_64x64_p64", "rm_64x64_p65_g", "rm_64x64_p256", "rm_37x53_p257_g",
                                  "rm_64x64_p1024", "rm_37x53_p1024_g", "rm_120x200_p256", "rm_120x200_p257_g",
                                  "rm_120x200_U16", "rm_grey_U8", "rm_grey_U27", "rm_grey_U64_g", "rm_dup_p17",
                                  "rm_mediancut_16", "rm_mediancut_64_g"])
def test_cpu_restatement_matches_reference(rm_json, rm_npz, name):
    case = next(c for c in rm_json["cases"] if c["name"] == name)
    assert case["h"] * case["w"] <= 300 * 300
    arr = rm_input(case["input"])
    got = riemersma_ref.apply(arr, [tuple(c) for c in case["palette"]], case["use_gamma"])
    if case.get("full"):
        assert np.array_equal(got, rm_npz["out_" + name])
    assert sha(got) == case["output_sha256"]


def test_every_small_fixture_is_covered(rm_json):
    small = {c["name"] for c in rm_json["cases"] if c["h"] * c["w"] <= 300 * 300}
    params = test_cpu_restatement_matches_reference.pytestmark[0].args[1]
    assert small == set(params)


def test_strategy_plumbing(kat):
    from dither_pie_amd import dithering_lib as d
    s = d.ImageDitherer(16, d.DitherMode.RIEMERSMA)._get_dither_strategy(d.DitherMode.RIEMERSMA)
    assert isinstance(s, d.RiemersmaDitherStrategy) and isinstance(s, d.BaseDitherStrategy)
    assert s.get_current_parameters() == {}
    assert d.RiemersmaDitherStrategy.get_parameter_info() is None
    assert d.ImageDitherer.get_mode_parameters(d.DitherMode.RIEMERSMA) is None
    assert kat["misc"]["mode_parameters"]["riemersma"] is None
    assert not d.ImageDitherer.mode_has_parameters(d.DitherMode.RIEMERSMA)
    assert "RiemersmaDitherStrategy" in d.__all__
    with pytest.raises(ValueError):   # tiles / bands: the path crosses every boundary
        s._run(None, None, y0=4)
    with pytest.raises(ValueError):
        s._run(None, None, x0=1)
    for mode in (d.DitherMode.HALFTONE, d.DitherMode.WAVELET):
        with pytest.raises(NotImplementedError, match="riemersma"):
            d.ImageDitherer()._get_dither_strategy(mode)


def test_band_sharding_refuses_riemersma():
    from dither_pie_amd import dithering_lib as d, sharding
    assert d.DitherMode.RIEMERSMA not in d.ORDERED_MODES
    with pytest.raises(ValueError, match="does not shard"):
        sharding.dither_band(d.ImageDitherer(16, d.DitherMode.RIEMERSMA, [(0, 0, 0), (255, 255, 255)]), None, 10)


def test_c_abi_argument_errors_without_gpu(lib):
    from dither_pie_amd import _lib
    from dither_pie_amd._lib import DP_EINVAL, DP_OK
    assert "dp_riemersma_u8" in _lib.EXPORTS and hasattr(lib, "dp_riemersma_u8")
    assert lib.dp_version() == _lib.ABI_VERSION == 103
    # a stand-in palette handle of zeros, as long as tests/test_idiff_cpu.py makes its own: the entry point reads the palette's
    # metric field (0: RGB) before it looks at the sizes, and 64 bytes ended in front of that field
    fake = C.create_string_buffer(8192)
    pal = C.cast(fake, C.c_void_p)
    buf = C.cast(C.create_string_buffer(16), C.c_void_p)
    assert lib.dp_riemersma_u8(buf, buf, 1, 2, 2, None, None) == DP_EINVAL
    assert b"palette" in lib.dp_last_error()
    for n, h, w in ((-1, 2, 2), (1, -2, 2), (1, 2, -2)):
        assert lib.dp_riemersma_u8(buf, buf, n, h, w, pal, None) == DP_EINVAL
        assert b"negative" in lib.dp_last_error()
    assert lib.dp_riemersma_u8(None, buf, 1, 2, 2, pal, None) == DP_EINVAL
    assert b"NULL" in lib.dp_last_error()
    assert lib.dp_riemersma_u8(buf, None, 1, 2, 2, pal, None) == DP_EINVAL
    # nothing to do: OK, buffers may be NULL
    assert lib.dp_riemersma_u8(None, None, 0, 2, 2, pal, None) == DP_OK
    assert lib.dp_riemersma_u8(None, None, 3, 0, 2, pal, None) == DP_OK
