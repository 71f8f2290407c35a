"""GPU tier: the HIP kernels, called through the C ABI, against the oracle and the golden fixtures.

Bit-exact for every mode (ordered modes, palette assignment AND error diffusion: the decisions are
discrete, so anything but identical float32 sums would show up as different palette colours)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, case_input, case_palette

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "kat.json")) as _f:
    _KAT = json.load(_f)
_CASES = _KAT["cases"]


@pytest.fixture(scope="module")
def be():
    import torch
    from dither_pie_amd import backend
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return backend


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_case(be, orc, arr, pal, mode, params, gamma, y0=0, x0=0, accel=True):
    p = dict(orc.MODE_DEFAULTS[mode])
    p.update(params or {})
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, gamma)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=accel)
    x = _dev(arr)
    if mode == "none":
        out = be.ordered(x, P, be.MODE_NEAREST, y0=y0, x0=x0)
    elif mode == "bayer":
        out = be.ordered(x, P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(orc.bayer_matrix(p["size"])), y0=y0, x0=x0)
    elif mode == "polka_dot":
        out = be.ordered(x, P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(orc.polka_dot_matrix(p["tile_size"], p["gamma"])),
                         y0=y0, x0=x0)
    elif mode == "blue_noise":
        out = be.ordered(x, P, be.MODE_MATRIX, thr=be.Thresholds.blue_noise(p["size"], p["seed"]), y0=y0, x0=x0)
    elif mode == "IGN":
        out = be.ordered(x, P, be.MODE_IGN, ign_scale=p["scale"], ign_seed=p["seed"], y0=y0, x0=x0)
    elif mode == "error_diffusion":
        taps, div = orc.ed_kernel(p["variant"])
        out = be.error_diffusion(x, P, taps, div, p["serpentine"] == "true")
    elif mode == "perceptual":
        out = be.variable_diffusion(x, P, be.DIFFUSER_PERCEPTUAL)
    elif mode == "hybrid":
        out = be.variable_diffusion(x, P, be.DIFFUSER_HYBRID, p["lum_factor"], p["col_factor"])
    elif mode == "adaptive_variance":
        gate = be.variance_gate(x, P, p["var_threshold"], p["window_radius"])
        out = be.variable_diffusion(x, P, be.DIFFUSER_ADAPTIVE_VARIANCE, gate=gate)
    elif mode == "ostromoukhov":
        import torch
        coef = torch.from_numpy(orc.ostromoukhov_coefficients()).cuda()
        out = be.variable_diffusion(x, P, be.DIFFUSER_OSTROMOUKHOV, serpentine=(p["serpentine"] == "true"), coef=coef)
    else:
        raise ValueError(mode)
    return out.cpu().numpy()


def _assert_same(out, ref, what=""):
    if not np.array_equal(out, ref):
        bad = np.argwhere((out != ref).any(-1))
        raise AssertionError(f"{what}: {len(bad)} of {ref.shape[0] * ref.shape[1]} pixels differ, first {bad[:5].tolist()}")


@pytest.mark.parametrize("case", _CASES, ids=lambda c: c["name"])
def test_golden_cases(be, orc, gold, case):
    arr = case_input(orc, case["input"])
    pal = case_palette(orc, case["palette"])
    out = _run_case(be, orc, arr, pal, case["mode"], case["params"], case["gamma"])
    if case["full"]:
        _assert_same(out, gold["out_" + case["name"]], case["name"])
    assert orc.H(out) == case["h_out"]


@pytest.mark.parametrize("K,seed", [(2, 1), (3, 2), (10, 3), (11, 4), (16, 5), (57, 6), (128, 7), (256, 8)])
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "8x8"}), ("bayer", {"size": "2x2"}),
                                         ("IGN", {"scale": 1.7, "seed": 23}), ("blue_noise", {"size": 32, "seed": 5})])
def test_ordered_vs_oracle(be, orc, K, seed, mode, params):
    pal = orc.palr(K, seed)
    for arr in (orc.rnd(67, 93, seed), orc.grad(70, 131)):
        ref = orc.apply_dithering(arr, pal, mode, params, False)
        for accel in (True, False):  # LDS cell-table kernel and brute-force kernel
            out = _run_case(be, orc, arr, pal, mode, params, False, accel=accel)
            _assert_same(out, ref, f"{mode} K={K} accel={accel}")


def test_single_colour_palette(be, orc):
    arr = orc.rnd(20, 30, 1)
    for mode, params in [("none", {}), ("bayer", {}), ("IGN", {})]:
        out = _run_case(be, orc, arr, [(12, 200, 99)], mode, params, False)
        assert (out == np.array([12, 200, 99], np.uint8)).all()


def test_duplicate_palette_entries_all_ties(be, orc):
    pal = [(50, 60, 70)] * 3 + [(200, 10, 10)] * 2 + [(50, 60, 70)]
    arr = orc.grad(64, 80)
    for mode, params in [("none", {}), ("bayer", {"size": "4x4"})]:
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), mode)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (3, 5), (17, 33), (64, 64), (2, 1025)])
def test_ragged_shapes(be, orc, shape):
    arr = orc.rnd(shape[0], shape[1], 77)
    pal = orc.palr(32)
    for mode, params in [("none", {}), ("bayer", {"size": "16x16"}), ("IGN", {})]:
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), f"{mode} {shape}")


def test_batched_frames_and_tile_offsets(be, orc):
    import torch
    pal = orc.palr(64, 9)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    frames = np.stack([orc.rnd(45, 71, s) for s in range(5)])
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("8x8"))
    out = be.ordered(_dev(frames), P, be.MODE_MATRIX, thr=thr).cpu().numpy()
    for i in range(5):
        _assert_same(out[i], orc.apply_dithering(frames[i], pal, "bayer", {"size": "8x8"}), f"frame {i}")
    # row bands with global offsets reproduce the full image (config 4's tiling)
    big = orc.grad(96, 128)
    full = orc.apply_dithering(big, pal, "IGN", {"scale": 1.3, "seed": 5})
    for (ya, yb) in [(0, 33), (33, 64), (64, 96)]:
        o = be.ordered(_dev(big[ya:yb]), P, be.MODE_IGN, ign_scale=1.3, ign_seed=5, y0=ya).cpu().numpy()
        _assert_same(o, full[ya:yb], f"band {ya}")
    del torch


def test_unaligned_input_pointer(be, orc):
    import torch
    pal = orc.palr(16)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    arr = orc.rnd(31, 47, 3)
    buf = torch.empty(arr.size + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + arr.size].view(31, 47, 3)
    view.copy_(_dev(arr))
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    out = be.ordered(view, P, be.MODE_MATRIX, thr=thr).cpu().numpy()
    _assert_same(out, orc.apply_dithering(arr, pal, "bayer", {"size": "4x4"}), "unaligned")


@pytest.mark.parametrize("size,seed", [(32, 42), (64, 42), (32, 0), (33, 9999), (96, 1), (128, 42), (130, 7)])
def test_blue_noise_on_device(be, gold, size, seed):
    bn = be.Thresholds.blue_noise(size, seed).numpy()
    assert np.array_equal(bn, gold[f"blue_{size}_{seed}"])


def test_ign_field(be, orc, gold):
    assert np.array_equal(be.ign_thresholds(8, 8, 1.0, 0).cpu().numpy(), gold["ign_8x8_s1_seed0"])
    assert np.array_equal(be.ign_thresholds(37, 53, 2.5, 17).cpu().numpy(), gold["ign_37x53_s25_seed17"])
    assert np.array_equal(be.ign_thresholds(64, 64, 0.1, 9999).cpu().numpy(), gold["ign_64x64_s01_seed9999"])
    assert orc.H(be.ign_thresholds(1080, 1920, 2.5, 17).cpu().numpy()) == _KAT["misc"]["ign_1080_s25_seed17"]


@pytest.mark.parametrize("variant", ["floyd_steinberg", "jjn", "stucki", "burkes", "atkinson", "sierra",
                                     "sierra_two_row", "sierra_lite"])
@pytest.mark.parametrize("serp", ["false", "true"])
def test_error_diffusion_vs_oracle(be, orc, variant, serp):
    for arr, pal in [(orc.rnd(150, 97, 4), orc.palr(16, 3)), (orc.grad(131, 200), orc.generate_uniform_palette(16)),
                     (orc.rnd(70, 40, 5), orc.palr(40, 9))]:
        params = {"variant": variant, "serpentine": serp}
        out = _run_case(be, orc, arr, pal, "error_diffusion", params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, "error_diffusion", params, False), f"{variant} {serp}")


@pytest.mark.parametrize("variant", ["floyd_steinberg", "jjn", "atkinson", "sierra_lite", "burkes"])
@pytest.mark.parametrize("serp", [False, True])
def test_error_diffusion_numba_arithmetic_vs_oracle(be, orc, variant, serp):
    """The reference's numba branch (dithering_lib.py:213-308, typed per numba's unification rule: float64 linear-scan
    nearest, float64 error, float64 pushes rounded on the store) through dp_error_diffusion_numba_u8 against its C restatement -- several bands, several frames, a palette with
    exact float32 ties (uniform) and one without, with and without the gamma table.  (That restatement is itself not
    pinned by reference output: numba is not installable here.)"""
    import torch
    for arr, pal, gamma in [(orc.rnd(150, 97, 4), orc.palr(16, 3), False), (orc.grad(131, 200), orc.generate_uniform_palette(16), False),
                            (orc.rnd(70, 40, 5), orc.palr(40, 9), True), (orc.rnd(9, 5, 6), orc.palr(2, 1), False)]:
        pal_f32, out_colors, lut_in = orc.prepare_palette(pal, gamma)
        P = be.Palette(pal_f32, out_colors, lut_in)
        taps, div = orc.ed_kernel(variant)
        frames = np.stack([arr, arr[::-1].copy()])
        out = be.error_diffusion(torch.from_numpy(frames).cuda(), P, taps, div, serp, arithmetic="numba").cpu().numpy()
        for f in range(2):
            ref = orc.error_diffusion_numba_u8(frames[f], pal_f32, out_colors, lut_in, variant, serp)
            _assert_same(out[f], ref, f"numba arithmetic {variant} serp={serp} frame {f}")


@pytest.mark.gpu
def test_numba_fixtures_on_the_device_when_present(be, orc):
    """SURVEY row a7 on the device: dp_error_diffusion_numba_u8 / dp_hybrid_numba_u8 against what the REFERENCE's numba branches
    produced (tests/golden/numba.*, recorded by make_golden.py --numba on a host that has numba).  Skips with 'unpinned' while
    nobody has recorded them -- the kernels are then checked against the (equally unpinned) C restatement only."""
    import torch
    from conftest import case_input, case_palette, numba_fixtures
    fx = numba_fixtures()
    if fx is None:
        pytest.skip("a7 parity UNPINNED on the device too: tests/golden/numba.{json,npz} absent")
    rec, arrs = fx
    for c in rec["cases"]:
        arr, pal = case_input(orc, c["input"]), case_palette(orc, c["palette"])
        P = be.Palette(*orc.prepare_palette(pal, c["gamma"]))
        x = torch.from_numpy(arr).cuda()
        if c["kind"] == "error_diffusion":
            taps, div = orc.ed_kernel(c["params"]["variant"])
            out = be.error_diffusion(x, P, taps, div, c["params"]["serpentine"] == "true", arithmetic="numba")
        else:
            out = be.hybrid_numba(x, P, c["params"]["lum_factor"], c["params"]["col_factor"])
        _assert_same(out.cpu().numpy(), arrs[c["name"]], c["name"])


def test_error_diffusion_numba_float64_reading(be, orc):
    """The probe of tests/test_oracle_golden.py::test_numba_branch_follows_float64_unification on the device: the kernel
    takes the entry that is nearer in float64 (numba unifies r to float64), not the one a float32 scan collapses onto; and a
    strip with tiny values against far colours (float64 errors that float32 cannot hold) equals the restatement on both
    kernels (wavefront / frame-parallel serpentine)."""
    import torch
    from test_oracle_golden import _numba_reading_probe
    arr, pal_f32, out_colors = _numba_reading_probe()
    P = be.Palette(pal_f32, out_colors, None)
    taps, div = orc.ed_kernel("floyd_steinberg")
    out = be.error_diffusion(torch.from_numpy(arr).cuda(), P, taps, div, False, arithmetic="numba").cpu().numpy()
    assert out[0, 0].tolist() == [200, 210, 220]
    assert orc.error_diffusion_numba_numpy(arr, pal_f32, out_colors, None, "floyd_steinberg", False, scan="float32")[0, 0].tolist() == [10, 20, 30]
    pal2 = np.array([[255.0, 255.0, 255.0], [0.3, 0.3, 0.3], [17.7, 200.1, 3.3]], np.float32)
    oc2 = np.array([[255, 255, 255], [0, 0, 0], [18, 200, 3]], np.uint8)
    P2 = be.Palette(pal2, oc2, None)
    taps, div = orc.ed_kernel("jjn")
    for shape, seed in [((3, 40), 8), ((200, 333), 9), ((70, 1), 10)]:
        strip = orc.rnd(shape[0], shape[1], seed)
        for serp in (False, True):
            out = be.error_diffusion(torch.from_numpy(strip).cuda(), P2, taps, div, serp, arithmetic="numba").cpu().numpy()
            _assert_same(out, orc.error_diffusion_numba_u8(strip, pal2, oc2, None, "jjn", serp), f"numba float64 {shape} serp={serp}")


@pytest.mark.gpu
@pytest.mark.parametrize("lum_factor,col_factor", [(1.0, 0.2), (1.4, 0.0), (0.3, 1.0)])
def test_hybrid_numba_arithmetic_vs_oracle(be, orc, lum_factor, col_factor):
    """HybridDitherStrategy's numba branch (_hybrid_numba, dithering_lib.py:1396-1494) through dp_hybrid_numba_u8 against its C
    restatement: several bands, frames in a batch, with and without the gamma table, one 1080p frame spread over workgroups; and
    through the strategy with ERROR_DIFFUSION_ARITHMETIC = "numba" (default: the pure-Python branch, pinned by fixtures).
    Unpinned like the other numba branch: numba is not installable here."""
    import torch
    from dither_pie_amd import dithering_lib as dl
    for arr, pal, gamma in [(orc.rnd(150, 97, 4), orc.palr(16, 3), False), (orc.grad(131, 200), orc.generate_uniform_palette(16), False),
                            (orc.rnd(70, 40, 5), orc.palr(40, 9), True), (orc.rnd(9, 5, 6), orc.palr(2, 1), False)]:
        pal_f32, out_colors, lut_in = orc.prepare_palette(pal, gamma)
        P = be.Palette(pal_f32, out_colors, lut_in)
        frames = np.stack([arr, arr[::-1].copy()])
        out = be.hybrid_numba(torch.from_numpy(frames).cuda(), P, lum_factor, col_factor).cpu().numpy()
        for f in range(2):
            _assert_same(out[f], orc.hybrid_numba_u8(frames[f], pal_f32, out_colors, lut_in, lum_factor, col_factor), f"hybrid numba frame {f}")
    arr = orc.rnd(1080, 1920, 12)
    pal = orc.generate_uniform_palette(16)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    ref = orc.hybrid_numba_u8(arr, pal_f32, out_colors, lut_in, lum_factor, col_factor)
    old = dl.ERROR_DIFFUSION_ARITHMETIC
    dl.ERROR_DIFFUSION_ARITHMETIC = "numba"
    try:
        d = dl.ImageDitherer(16, dl.DitherMode.HYBRID, pal, False, {"lum_factor": lum_factor, "col_factor": col_factor})
        out = d.apply_dithering_frames(torch.from_numpy(arr).cuda()).cpu().numpy()
    finally:
        dl.ERROR_DIFFUSION_ARITHMETIC = old
    _assert_same(out, ref, "hybrid numba, 1080p")
    d = dl.ImageDitherer(16, dl.DitherMode.HYBRID, pal, False, {"lum_factor": lum_factor, "col_factor": col_factor})
    py = d.apply_dithering_frames(torch.from_numpy(arr).cuda()).cpu().numpy()
    _assert_same(py, orc.apply_dithering(arr, pal, "hybrid", {"lum_factor": lum_factor, "col_factor": col_factor}), "hybrid python, 1080p")
    assert not np.array_equal(py, out)


def test_error_diffusion_numba_arithmetic_1080p_bands_over_workgroups(be, orc):
    """One 1080p frame (17 bands spread over workgroups, the few-frames schedule) and the strategy-level switch."""
    import torch
    from dither_pie_amd import dithering_lib as dl
    arr = orc.rnd(1080, 1920, 11)
    pal = orc.generate_uniform_palette(16)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    ref = orc.error_diffusion_numba_u8(arr, pal_f32, out_colors, lut_in, "floyd_steinberg", False)
    old = dl.ERROR_DIFFUSION_ARITHMETIC
    dl.ERROR_DIFFUSION_ARITHMETIC = "numba"
    try:
        d = dl.ImageDitherer(16, dl.DitherMode.ERROR_DIFFUSION, pal, False, {"variant": "floyd_steinberg", "serpentine": "false"})
        out = d.apply_dithering_frames(torch.from_numpy(arr).cuda()).cpu().numpy()
    finally:
        dl.ERROR_DIFFUSION_ARITHMETIC = old
    _assert_same(out, ref, "numba arithmetic, 1080p")
    # inputs on which the two arithmetics disagree (exact ties: lowest index against scipy's traversal order; even values
    # against a 4x4x4 lattice): the numba entry point follows the numba restatement, the default one the pure-Python branch
    lv = [0, 64, 128, 192, 255]
    for pal2, arr2 in [([(a, b, c) for a in lv for b in lv for c in lv], np.full((70, 16, 3), 32, np.uint8)),
                       ([(a, b, c) for a in lv[:4] for b in lv[:4] for c in lv[:4]],
                        (np.random.RandomState(0).randint(0, 128, (48, 48, 3)) * 2).astype(np.uint8))]:
        pf, oc, lut = orc.prepare_palette(pal2, False)
        P = be.Palette(pf, oc, lut)
        taps, div = orc.ed_kernel("floyd_steinberg")
        t = torch.from_numpy(arr2).cuda()
        nb = be.error_diffusion(t, P, taps, div, False, arithmetic="numba").cpu().numpy()
        py = be.error_diffusion(t, P, taps, div, False).cpu().numpy()
        ref_nb = orc.error_diffusion_numba_u8(arr2, pf, oc, lut, "floyd_steinberg", False)
        ref_py = orc.error_diffusion_u8(arr2, pf, oc, lut, "floyd_steinberg", False)
        assert len(pal2) != 125 or not np.array_equal(ref_nb, ref_py)  # (the constant frame on the 5x5x5 lattice: every pixel)
        _assert_same(nb, ref_nb, "numba arithmetic on a tie-rich input")
        _assert_same(py, ref_py, "python arithmetic on a tie-rich input")


def test_error_diffusion_batch_and_gamma(be, orc):
    pal = orc.palr(16, 3)
    frames = np.stack([orc.rnd(80, 60, s) for s in range(3)])
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, True)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    taps, div = orc.ed_kernel("floyd_steinberg")
    for serp in (False, True):
        out = be.error_diffusion(_dev(frames), P, taps, div, serp).cpu().numpy()
        for i in range(3):
            ref = orc.apply_dithering(frames[i], pal, "error_diffusion",
                                      {"variant": "floyd_steinberg", "serpentine": "true" if serp else "false"}, True)
            _assert_same(out[i], ref, f"frame {i} serp={serp}")


def test_kmeans_step(be, orc):
    import torch
    px = orc.rnd(211, 173, 6).reshape(-1, 3)
    centers = px[:32].astype(np.float64) + 0.25
    sums, counts, sumsq = be.kmeans_step(_dev(px), torch.from_numpy(centers).cuda())
    rs, rc, rin = orc.kmeans_step(px, centers)
    assert np.array_equal(sums.cpu().numpy(), rs) and np.array_equal(counts.cpu().numpy(), rc)
    c = torch.from_numpy(centers)
    inertia = float((sumsq.cpu().double() - 2 * (c * sums.cpu().double()).sum(1) + counts.cpu().double() * (c * c).sum(1)).sum())
    assert abs(inertia - rin) <= 1e-9 * rin


def test_resize_nearest_matches_pillow(be, orc):
    from PIL import Image
    arr = orc.rnd(97, 131, 8)
    for (oh, ow) in [(48, 65), (194, 262), (33, 131), (97, 50), (291, 393), (16, 22), (27, 36), (1, 1), (5, 400)]:
        ref = np.array(Image.fromarray(arr).resize((ow, oh), Image.NEAREST))
        out = be.resize_nearest(_dev(arr), oh, ow).cpu().numpy()
        assert np.array_equal(out, ref), (oh, ow)
    frames = np.stack([orc.rnd(60, 80, s) for s in range(3)])
    out = be.resize_nearest(_dev(frames), 16, 22).cpu().numpy()
    for i in range(3):
        assert np.array_equal(out[i], np.array(Image.fromarray(frames[i]).resize((22, 16), Image.NEAREST)))


def test_resize_nearest_sweep_matches_pillow(be, orc):
    """The geometries the video path produces (video_processor.py:547-577, 393-420): 1080p / 4K / odd sources down to max_size
    32..256 on the smaller side (even dimensions) and back up by 2..8, plus 60 random size pairs -- Pillow's NEAREST decides."""
    from PIL import Image
    from dither_pie_amd.video_processor import _even_dimensions, _final_size
    rs = np.random.RandomState(77)
    pairs = []
    for (h, w) in [(1080, 1920), (2160, 3840), (719, 1279), (480, 853), (1920, 1080)]:
        for ms in (32, 64, 100, 127, 256):
            tw, th = _even_dimensions(w, h, ms)
            pairs.append((h, w, th, tw))
            for m in (2, 3, 8):
                nw, nh = _final_size(tw, th, m)
                pairs.append((th, tw, nh, nw))
    for _ in range(60):
        pairs.append((int(rs.randint(1, 700)), int(rs.randint(1, 900)), int(rs.randint(1, 900)), int(rs.randint(1, 1100))))
    for (h, w, oh, ow) in pairs:
        arr = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        ref = np.array(Image.fromarray(arr).resize((ow, oh), Image.NEAREST))
        out = be.resize_nearest(_dev(arr), oh, ow).cpu().numpy()
        assert np.array_equal(out, ref), (h, w, oh, ow)


def test_accelerator_is_built_for_integer_and_float_palettes(be, orc):
    P = be.Palette(*orc.prepare_palette(orc.palr(256), False), accel=True)
    assert P.is_integer and P.accel_entries > 0 and 4 <= P.accel_max_list <= 64
    Pg = be.Palette(*orc.prepare_palette(orc.palr(256), True), accel=True)  # use_gamma: float coordinates + lut_in
    assert not Pg.is_integer and Pg.accel_entries > 0 and 4 <= Pg.accel_max_list <= 64
    Ps = be.Palette(*orc.prepare_palette(orc.palr(5), True), accel=True)     # too small to be worth a table
    assert Ps.accel_entries == 0


@pytest.mark.parametrize("K,seed", [(8, 1), (16, 2), (64, 3), (200, 4), (256, 5)])
def test_tie_heavy_inputs(be, orc, K, seed):
    """every pixel sits on a bisector of two palette colours (midpoints), or on a palette colour"""
    pal = orc.palr(K, seed)
    P = np.array(pal)
    rs = np.random.RandomState(seed)
    a, b = P[rs.randint(0, K, 6000)], P[rs.randint(0, K, 6000)]
    pts = np.concatenate([(a + b) // 2, (a + b + 1) // 2, P[rs.randint(0, K, 1000)]]).astype(np.uint8)
    arr = pts[: (len(pts) // 100) * 100].reshape(-1, 100, 3)
    for mode, params in [("none", {}), ("bayer", {"size": "8x8"}), ("IGN", {}), ("blue_noise", {"size": 32, "seed": 0})]:
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), f"{mode} K={K}")


def test_clustered_palette_long_lists(be, orc):
    rs = np.random.RandomState(3)
    pal = [tuple(int(v) for v in np.clip(rs.normal(128, 6, 3), 0, 255)) for _ in range(200)] + orc.palr(56, 2)
    arr = np.clip(rs.normal(128, 10, (90, 120, 3)), 0, 255).astype(np.uint8)
    for mode, params in [("none", {}), ("bayer", {"size": "4x4"})]:
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), mode)


def test_empty_batch_and_degenerate_shapes(be, orc):
    import torch
    P = be.Palette(*orc.prepare_palette(orc.palr(16), False), accel=True)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    empty = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda")
    assert be.ordered(empty, P, be.MODE_MATRIX, thr=thr).shape == (0, 8, 8, 3)
    taps, div = orc.ed_kernel("floyd_steinberg")
    assert be.error_diffusion(empty, P, taps, div).shape == (0, 8, 8, 3)
    for shape in [(1, 9001), (3, 4097), (4099, 2)]:  # wider than a 4096-pixel tile, very tall and thin
        arr = orc.rnd(shape[0], shape[1], 5)
        for mode, params in [("bayer", {"size": "16x16"}), ("IGN", {"scale": 0.3, "seed": 9})]:
            out = _run_case(be, orc, arr, orc.palr(16), mode, params, False)
            _assert_same(out, orc.apply_dithering(arr, orc.palr(16), mode, params, False), f"{mode} {shape}")


def test_full_size_properties_and_2g_pixel_chunking(be, orc):
    """BASELINE sizes through size-independent properties: every copy of a frame in a > 2^31-pixel batch
    (the launcher splits such batches) dithers to the bytes of the single-frame call, whose hash is the KAT;
    the output only uses palette colours; dithering is idempotent for mode 'none'."""
    import hashlib
    import torch
    free, _ = torch.cuda.mem_get_info()
    n = 260  # 260 * 3840 * 2160 = 2.157e9 pixels > 2^31
    if free < 2.2 * n * 2160 * 3840 * 3:
        pytest.skip("not enough free HBM")
    pal = orc.palr(256)
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("8x8"))
    frame = _dev(orc.rnd(2160, 3840, 1234))
    single = be.ordered(frame, P, be.MODE_MATRIX, thr=thr)
    assert hashlib.sha256(single.cpu().numpy().tobytes()).hexdigest()[:16] == "7041bd52fdea90b5"
    batch = frame.unsqueeze(0).expand(n, -1, -1, -1).contiguous()
    out = be.ordered(batch, P, be.MODE_MATRIX, thr=thr)
    del batch
    for i in (0, 1, 127, 128, 129, 255, 256, 259):  # around the chunk boundary too
        assert torch.equal(out[i], single), i
    assert bool((out == single.unsqueeze(0)).all())
    del out
    # palette closure + idempotence of nearest-colour assignment at 4K
    near = be.ordered(frame, P, be.MODE_NEAREST)
    packed = (near[..., 0].to(torch.int64) << 16) | (near[..., 1].to(torch.int64) << 8) | near[..., 2].to(torch.int64)
    palset = torch.tensor([(r << 16) | (g << 8) | b for r, g, b in pal], device="cuda")
    assert bool(torch.isin(packed, palset).all())
    assert torch.equal(be.ordered(near, P, be.MODE_NEAREST), near)


@pytest.mark.parametrize("K,seed", [(257, 1), (300, 2), (700, 3), (1024, 4)])
def test_large_palettes(be, orc, K, seed):
    """above 256 colours: brute-force kernels with the 10-bit index key and the large traversal queue"""
    pal = orc.palr(K, seed)
    for arr in (orc.rnd(40, 61, seed), orc.grad(64, 80)):
        for mode, params in [("none", {}), ("bayer", {"size": "8x8"}), ("IGN", {}), ("blue_noise", {"size": 32, "seed": 2})]:
            out = _run_case(be, orc, arr, pal, mode, params, False)
            _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), f"{mode} K={K}")
    arr = orc.rnd(70, 45, seed)
    for params in [{"variant": "floyd_steinberg", "serpentine": "false"}, {"variant": "atkinson", "serpentine": "true"}]:
        out = _run_case(be, orc, arr, pal, "error_diffusion", params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, "error_diffusion", params, False), f"ed K={K}")
    out = _run_case(be, orc, orc.grad(33, 47), pal, "bayer", {"size": "4x4"}, True)
    _assert_same(out, orc.apply_dithering(orc.grad(33, 47), pal, "bayer", {"size": "4x4"}, True), f"gamma K={K}")


@pytest.mark.parametrize("mode,params", [("perceptual", {}), ("hybrid", {"lum_factor": 1.4, "col_factor": 0.0}),
                                         ("adaptive_variance", {"var_threshold": 120.0, "window_radius": 3}),
                                         ("ostromoukhov", {"serpentine": "false"}), ("ostromoukhov", {"serpentine": "true"})])
def test_variable_diffusers_vs_oracle(be, orc, mode, params):
    for arr, pal in [(orc.rnd(70, 45, 4), orc.palr(16, 3)), (orc.grad(60, 90), orc.generate_uniform_palette(27)),
                     (orc.rnd(33, 64, 5), orc.palr(300, 9))]:
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), f"{mode}")
    frames = np.stack([orc.rnd(40, 50, s) for s in range(70)])  # more frames than lanes of one wave
    import torch
    P = be.Palette(*orc.prepare_palette(orc.palr(16, 3), False))
    if mode == "perceptual":
        out = be.variable_diffusion(_dev(frames), P, be.DIFFUSER_PERCEPTUAL).cpu().numpy()
        for i in (0, 1, 63, 64, 69):
            _assert_same(out[i], orc.apply_dithering(frames[i], orc.palr(16, 3), mode, params, False), f"frame {i}")


def test_variance_gate_matches_scipy_restatement(be, orc):
    arr = orc.rnd(77, 91, 3)
    for gamma in (False, True):
        pal_f32, oc, lut = orc.prepare_palette(orc.palr(16), gamma)
        P = be.Palette(pal_f32, oc, lut)
        src = lut[arr] if lut is not None else arr
        for thr, rad in [(300.0, 1), (50.0, 2), (900.0, 5)]:
            gate = be.variance_gate(_dev(arr), P, thr, rad).cpu().numpy()[0]
            ref, _ = orc.variance_gate(src, thr, rad)
            assert np.array_equal(gate, ref), (gamma, thr, rad)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "8x8"}), ("bayer", {"size": "2x2"}),
                                         ("blue_noise", {"size": 32, "seed": 3}), ("IGN", {"scale": 1.5, "seed": 4}),
                                         ("polka_dot", {"tile_size": 8, "gamma": 1.5}),
                                         ("polka_dot", {"tile_size": 6, "gamma": 0.8}),   # not a power of two
                                         ("blue_noise", {"size": 33, "seed": 5})])
@pytest.mark.parametrize("w", [1003, 1004])
def test_lean_kernel_queue_drains_and_row_straddles(be, orc, mode, params, w):
    """The lean kernel defers split cells, ties and row-straddling groups to its wave-private queue; a frame
    with many tie colours, an odd width and a tile origin makes every wave drain the queue several times.
    Checked against the oracle and against the brute-force kernels (no accelerator)."""
    rs = np.random.RandomState(77)
    pal = orc.palr(256, seed=21)
    arr = orc.rnd(611, w, 5)
    # a third of the pixels are exact palette colours or midpoints of palette pairs (distance ties)
    pick = rs.randint(0, 256, (611, w))
    mid = (np.asarray(pal)[pick].astype(np.int64) + np.asarray(pal)[(pick + 1) % 256]) // 2
    sel = rs.randint(0, 3, (611, w, 1))
    arr = np.where(sel == 0, mid.astype(np.uint8), arr)
    ref = orc.apply_dithering(arr, pal, mode, params, False, y0=5, x0=3)
    out = _run_case(be, orc, arr, pal, mode, params, False, y0=5, x0=3)
    _assert_same(out, ref, f"lean {mode} w={w}")
    out2 = _run_case(be, orc, arr, pal, mode, params, False, y0=5, x0=3, accel=False)
    _assert_same(out2, ref, f"brute {mode} w={w}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "8x8"}), ("blue_noise", {"size": 32, "seed": 3}),
                                         ("IGN", {"scale": 1.5, "seed": 4}), ("polka_dot", {"tile_size": 5, "gamma": 1.5})])
@pytest.mark.parametrize("K,w", [(256, 1003), (64, 1004), (9, 640)])
def test_float_palette_cell_table(be, orc, mode, params, K, w):
    """use_gamma palettes (float32 coordinates, pixels through lut_in) on their own cell table: float32 ranking
    with a 128-ulp certainty gap, float64 recomputation of the two winners; near ties go to the fix-up pass.
    Checked against the oracle and the float64 brute-force kernel."""
    rs = np.random.RandomState(78)
    pal = orc.palr(K, seed=31)
    arr = orc.rnd(411, w, 6)
    pick = rs.randint(0, K, (411, w))
    arr = np.where(rs.randint(0, 4, (411, w, 1)) == 0, np.asarray(pal, dtype=np.uint8)[pick], arr)  # exact palette hits
    ref = orc.apply_dithering(arr, pal, mode, params, True, y0=2, x0=7)
    pal_f32, oc, lut = orc.prepare_palette(pal, True)
    P = be.Palette(pal_f32, oc, lut, accel=True)
    assert P.accel_entries > 0, "the float accelerator should have been built"
    out = _run_case(be, orc, arr, pal, mode, params, True, y0=2, x0=7)
    _assert_same(out, ref, f"float table {mode} K={K} w={w}")
    out2 = _run_case(be, orc, arr, pal, mode, params, True, y0=2, x0=7, accel=False)
    _assert_same(out2, ref, f"float brute {mode} K={K} w={w}")


@pytest.mark.gpu
@pytest.mark.parametrize("K,gamma", [(256, False), (256, True), (97, False), (9, False), (200, True)])
@pytest.mark.parametrize("variant,serp", [("floyd_steinberg", "false"), ("jjn", "false"), ("atkinson", "true")])
def test_error_diffusion_candidate_lists(be, orc, K, gamma, variant, serp):
    """Palettes of 9..256 colours search only the cell's candidate list (entries that can be nearest to some point
    of the 8x8x8 cell); the result must stay bit-exact, including clustered palettes (long lists) and duplicates."""
    rs = np.random.RandomState(K)
    pal = orc.palr(K, seed=K + 5)
    if K == 97:  # a tight cluster (lists longer than 15 -> full scan) plus duplicates
        pal = pal[:60] + [(120 + int(a), 121 + int(b), 119 + int(c)) for a, b, c in rs.randint(0, 4, (30, 3))] + pal[:7]
    arr = orc.rnd(96, 161, 11)
    arr[20:60, 30:90] = np.asarray(pal, dtype=np.uint8)[rs.randint(0, len(pal), (40, 60))]
    params = {"variant": variant, "serpentine": serp}
    out = _run_case(be, orc, arr, pal, "error_diffusion", params, gamma)
    _assert_same(out, orc.apply_dithering(arr, pal, "error_diffusion", params, gamma), f"K={K} gamma={gamma} {variant}")


@pytest.mark.gpu
def test_serpentine_wide_rows_use_the_frame_parallel_kernel(be, orc):
    """The one-wave-per-frame serpentine kernel keeps three error rows in LDS (rows up to ~4400 pixels); wider rows
    fall back to the lane = frame kernel with its error rows in global memory.  Same bytes either way."""
    pal = orc.palr(16, 3)
    for w in (4300, 5001):
        arr = orc.rnd(5, w, w)
        params = {"variant": "sierra", "serpentine": "true"}
        out = _run_case(be, orc, arr, pal, "error_diffusion", params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, "error_diffusion", params, False), f"w={w}")


@pytest.mark.gpu
def test_ostromoukhov_serpentine_wide_rows(be, orc):
    """Ostromoukhov's serpentine scan keeps two error rows of four floats and its 768 coefficients in LDS while
    (8 w + 768) * 4 + 512 <= 158 * 1024 for palettes of up to 64 colours: w = 4900 needs 160 384 bytes of the 161 792 and
    runs one wave per frame, w = 5001 needs 163 616 and runs the lane = frame kernel with its error rows in global memory.
    (Which kernel ran cannot be seen from here and is not asserted.)  Same bytes as the oracle either way, with a whole-palette
    scan that ends in an exact tie at pixel (0, 0): no error has arrived there, so the query is the pixel itself, the midpoint
    of two entries of a 40-colour palette -- above the KD-tree's leaf size, so the tie replays the tree.  (The tie is exact
    without gamma only: under gamma the query is the linearised pixel among linearised entries, which need not tie; those
    cases check the two kernels' bytes all the same.  The frame's seed is its width.)"""
    tie_a, tie_b = (100, 100, 100), (104, 100, 100)
    mid = (102, 100, 100)
    pal40 = orc.palr(38, 5) + [tie_a, tie_b]
    d = ((np.array(pal40, np.int64) - np.array(mid, np.int64)) ** 2).sum(1)
    assert sorted(np.argsort(d, kind="stable")[:2].tolist()) == [38, 39] and d[38] == d[39] and np.sort(d)[2] > d[38]
    params = {"serpentine": "true"}
    for w in (4900, 5001):
        arr = orc.rnd(5, w, w)
        arr[0, 0] = mid
        for pal in (orc.palr(16, 3), pal40):
            for gamma in (False, True):
                out = _run_case(be, orc, arr, pal, "ostromoukhov", params, gamma)
                _assert_same(out, orc.apply_dithering(arr, pal, "ostromoukhov", params, gamma), f"w={w} K={len(pal)} gamma={gamma}")


def _fuzz_ordered():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_ordered.py")
    spec = importlib.util.spec_from_file_location("fuzz_ordered", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12])
def test_randomised_cases_against_oracle(be, orc, switches, seed):
    """150 random (mode, parameters, palette size, gamma, shape, tile origin, tie-rich content) cases per seed, each with a
    forced cell table and, one in three, the compact kernel forced onto it (DP_* switches: the twin library)."""
    assert _fuzz_ordered().run(seed, 150) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [13, 14, 15])
def test_randomised_cases_against_oracle_product_library(be, orc, seed):
    """The same generator on the library that ships: 150 cases per seed, tables / kernels chosen by the library itself."""
    from dither_pie_amd import _lib
    assert not _lib.EXPERIMENTS
    assert _fuzz_ordered().run(seed, 150, force=False) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22])
def test_randomised_diffusion_cases_against_oracle(be, orc, seed):
    """150 random diffusion cases per seed: the eight tap sets, both scans, both arithmetics, the four variable-coefficient
    diffusers; palette sizes around every table boundary, uniform / random / clustered palettes, gamma, shapes from 1x1 to
    a few bands, batches (tests/fuzz_diffusion.py)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_diffusion.py")
    spec = importlib.util.spec_from_file_location("fuzz_diffusion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(seed, 150) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 5, 7, 8, 16, 27, 64])
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "4x4"}), ("IGN", {})])
def test_small_palettes_four_entry_blocks(be, orc, K, mode, params):
    """Palettes of up to 64 colours get a table of 4-entry blocks when few cells overflow.  Uniform grids are the
    hard case: colours equidistant from many entries (cube centres, face centres) overflow any block and are
    resolved by a scan of the whole palette inside the deferred path.  Frames mix noise with exactly such points."""
    pal = orc.generate_uniform_palette(K) if K >= 8 else [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255),
                                                           (128, 128, 128), (64, 64, 64)][:K]
    pa = np.asarray(pal, dtype=np.int64)
    rs = np.random.RandomState(K)
    h, w = 300, 404
    arr = orc.rnd(h, w, K)
    i, j, k = rs.randint(0, len(pal), (3, h, w))
    mid2 = ((pa[i] + pa[j]) // 2).astype(np.uint8)
    mid3 = ((pa[i] + pa[j] + pa[k]) // 3).astype(np.uint8)
    cube = np.clip((pa[i] + 43) - (pa[i] + 43) % 85 + 42, 0, 255).astype(np.uint8)
    pick = rs.randint(0, 4, (h, w, 1))
    arr = np.where(pick == 0, mid2, np.where(pick == 1, mid3, np.where(pick == 2, cube, arr)))
    out = _run_case(be, orc, arr, pal, mode, params, False, y0=1, x0=2)
    _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False, y0=1, x0=2), f"uniform{K} {mode}")
    pal2 = orc.palr(K, seed=K + 1)  # random palette of the same size
    out = _run_case(be, orc, arr, pal2, mode, params, False)
    _assert_same(out, orc.apply_dithering(arr, pal2, mode, params, False), f"random{K} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "8x8"}), ("blue_noise", {"size": 32, "seed": 1})])
def test_clustered_palette_spills_split_nodes_to_global_memory(be, orc, mode, params):
    """A palette as median cut produces it for smooth content: most of its 256 colours sit in a few 16^3 cells, which
    need hundreds of split nodes -- more than LDS holds next to the 4096 cell blocks.  The deepest nodes then stay in
    global memory and only the deferred path reads them.  Content concentrated in exactly those cells."""
    rs = np.random.RandomState(9)
    dense = [(int(60 + a), int(100 + b), int(150 + c)) for a, b, c in rs.randint(0, 40, (216, 3))]
    pal = dense + orc.palr(40, seed=4)
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    assert P.accel_entries == 4096 * 8 + 88 * 64, "expected a table larger than LDS (staged part only)"
    h, w = 200, 301
    arr = np.clip(np.stack([60 + rs.randint(-8, 48, (h, w)), 100 + rs.randint(-8, 48, (h, w)), 150 + rs.randint(-8, 48, (h, w))], -1),
                  0, 255).astype(np.uint8)
    arr[:40] = orc.rnd(40, w, 3)
    out = _run_case(be, orc, arr, pal, mode, params, False, y0=3, x0=1)
    _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False, y0=3, x0=1), f"spilled table {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,serp,gamma", [("floyd_steinberg", "false", False), ("stucki", "false", True), ("burkes", "true", False)])
def test_error_diffusion_clustered_palette_refined_cells(be, orc, variant, serp, gamma):
    """216 of 256 colours inside a 40^3 cube: the 8^3 candidate cells there overflow their 15 entries and are refined
    down to unit cubes (host-built octree below each crowded cell); content inside and outside the crowded region."""
    rs = np.random.RandomState(9)
    dense = [(int(60 + a), int(100 + b), int(150 + c)) for a, b, c in rs.randint(0, 40, (216, 3))]
    pal = dense + orc.palr(40, seed=4)
    h, w = 70, 131
    arr = np.clip(np.stack([60 + rs.randint(-8, 48, (h, w)), 100 + rs.randint(-8, 48, (h, w)), 150 + rs.randint(-8, 48, (h, w))], -1),
                  0, 255).astype(np.uint8)
    arr[:20] = orc.rnd(20, w, 3)
    params = {"variant": variant, "serpentine": serp}
    out = _run_case(be, orc, arr, pal, "error_diffusion", params, gamma)
    _assert_same(out, orc.apply_dithering(arr, pal, "error_diffusion", params, gamma), f"clustered {variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("none", {}), ("bayer", {"size": "8x8"}), ("IGN", {})])
def test_clustered_float_palette_spills_split_nodes(be, orc, mode, params):
    """use_gamma with a clustered palette: the float cell table also keeps its deepest split nodes in global memory."""
    rs = np.random.RandomState(10)
    dense = [(int(90 + a), int(120 + b), int(160 + c)) for a, b, c in rs.randint(0, 44, (216, 3))]
    pal = dense + orc.palr(40, seed=6)
    pal_f32, oc, lut = orc.prepare_palette(pal, True)
    P = be.Palette(pal_f32, oc, lut, accel=True)
    assert P.accel_entries > 0
    h, w = 160, 203
    arr = np.clip(np.stack([90 + rs.randint(-10, 54, (h, w)), 120 + rs.randint(-10, 54, (h, w)), 160 + rs.randint(-10, 54, (h, w))], -1),
                  0, 255).astype(np.uint8)
    arr[:30] = orc.rnd(30, w, 3)
    out = _run_case(be, orc, arr, pal, mode, params, True, y0=2, x0=5)
    _assert_same(out, orc.apply_dithering(arr, pal, mode, params, True, y0=2, x0=5), f"float spilled {mode}")


def _image_like(rs, h, w, kind):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "dark":
        chans = [20 + 25 * np.sin(x / 12.0) ** 2 + 15 * (y / h), 18 + 22 * np.cos(y / 9.0) ** 2, 25 + 30 * np.sin((x + y) / 15.0) ** 2]
    else:
        chans = [80 + 60 * np.sin(x / 30.0) + 40 * (y / h), 110 + 50 * np.cos(y / 20.0) + 20 * np.sin(x / 9.7),
                 160 + 70 * (y / h) + 10 * np.sin((x + y) / 5.0)]
    return np.clip(np.stack(chans, -1) + rs.normal(0, 3, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["", "u4", "u8", "w4", "w8"])
@pytest.mark.parametrize("kind,K", [("dark", 8), ("dark", 16), ("smooth", 64), ("dark", 256), ("smooth", 256)])
def test_image_derived_palettes_every_cell_table(be, orc, switches, table, kind, K):
    """Palettes extracted from the image itself crowd a few cells of the plain 16^3 grid; the accelerator then builds its
    table over warped cells (per-channel maps staged in LDS).  Every table variant the accelerator can choose -- plain or
    warped cells, 4- or 8-entry blocks (DP_FORCE_TABLE; "" = its own choice) -- has to give the oracle's bytes, on the
    image-like content the palette came from and on noise (which lands in the wide cells of the warped grid)."""
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    if table:
        switches.setenv("DP_FORCE_TABLE", table)
    rs = np.random.RandomState(K + len(kind))
    h, w = 120, 203
    arr = _image_like(rs, h, w, kind)
    pal = ColorReducer.reduce_colors(Image.fromarray(arr, "RGB"), K)
    arr[:24] = orc.rnd(24, w, K)  # noise rows
    arr[24:30] = np.asarray(pal, dtype=np.uint8)[rs.randint(0, len(pal), (6, w))]  # exact palette colours
    for mode, params in (("none", {}), ("bayer", {"size": "8x8"}), ("IGN", {}), ("blue_noise", {"size": 32, "seed": 2})):
        out = _run_case(be, orc, arr, pal, mode, params, False, y0=2, x0=3)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False, y0=2, x0=3), f"{kind} K={K} table={table or 'auto'} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,K,gamma", [("floyd_steinberg", 16, False), ("jjn", 40, False), ("atkinson", 256, True)])
def test_error_diffusion_frame_spread_over_workgroups(be, orc, switches, variant, K, gamma):
    """Few frames in flight and at least four 64-row bands: the bands of a frame are spread over several workgroups that
    meet through progress words in global memory (agent-scope stores for the boundary rows).  Same bytes as the oracle and
    as the one-workgroup-per-frame schedule (DP_ED_ONE_WG=1)."""
    import torch
    h, w = 333, 150  # 6 bands, the last one partial
    arr = orc.rnd(h, w, K + 5)
    pal = orc.generate_uniform_palette(16) if K == 16 else orc.palr(K, seed=K)
    params = {"variant": variant, "serpentine": "false"}
    ref = orc.apply_dithering(arr, pal, "error_diffusion", params, gamma)
    out = _run_case(be, orc, arr, pal, "error_diffusion", params, gamma)
    _assert_same(out, ref, f"spread {variant}")
    switches.setenv("DP_ED_ONE_WG", "1")
    out1 = _run_case(be, orc, arr, pal, "error_diffusion", params, gamma)
    _assert_same(out1, ref, f"one workgroup {variant}")
    switches.delenv("DP_ED_ONE_WG")
    # a small batch: three different frames
    taps, div = orc.ed_kernel(variant)
    frames = np.stack([arr, orc.rnd(h, w, K + 6), orc.rnd(h, w, K + 7)])
    P = be.Palette(*orc.prepare_palette(pal, gamma), accel=True)
    got = be.error_diffusion(torch.from_numpy(frames).cuda(), P, taps, div, False).cpu().numpy()
    for i in range(3):
        _assert_same(got[i], orc.apply_dithering(frames[i], pal, "error_diffusion", params, gamma), f"batch frame {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,K,gamma,grid", [("floyd_steinberg", 16, False, 2), ("atkinson", 12, True, 3), ("jjn", 40, False, 1),
                                                  ("sierra_lite", 256, False, 4)])
def test_error_diffusion_persistent_workgroups(be, orc, switches, variant, K, gamma, grid):
    """More frames than workgroups (DP_ED_GRID forces what a batch larger than the number of CUs gets): a workgroup does every
    grid-th frame and its waves run on into the next frame's bands by a running band number -- frames of 6 and of 5 bands (the
    running number then changes which wave owns which band from frame to frame), the last band partial.  Same bytes as the
    oracle for every frame, and as one workgroup per frame."""
    import torch
    taps, div = orc.ed_kernel(variant)
    pal = orc.generate_uniform_palette(K) if K <= 16 else orc.palr(K, seed=K)
    params = {"variant": variant, "serpentine": "false"}
    for h, w, n in ((333, 90, 7), (290, 61, 9)):
        frames = np.stack([orc.rnd(h, w, 100 * K + i) for i in range(n)])
        P = be.Palette(*orc.prepare_palette(pal, gamma), accel=True)
        t = torch.from_numpy(frames).cuda()
        switches.setenv("DP_ED_ONE_WG", "1")  # (few frames: keep one workgroup per frame, the schedule a large batch has)
        one = be.error_diffusion(t, P, taps, div, False).cpu().numpy()
        switches.setenv("DP_ED_GRID", str(grid))
        got = be.error_diffusion(t, P, taps, div, False).cpu().numpy()
        switches.delenv("DP_ED_GRID")
        for i in range(n):
            ref = orc.apply_dithering(frames[i], pal, "error_diffusion", params, gamma)
            _assert_same(got[i], ref, f"persistent grid {grid}, {variant}, frame {i} of {n} ({h}x{w})")
            _assert_same(one[i], ref, f"one workgroup per frame, {variant}, frame {i}")


@pytest.mark.gpu
def test_error_diffusion_more_frames_than_compute_units(be, orc):
    """The product library on a batch larger than the device has CUs (what a video is): the persistent grid it chooses by
    itself.  330 small frames of six bands; every frame against the oracle."""
    import torch
    n, h, w = 330, 340, 24
    frames = np.stack([orc.rnd(h, w, 9000 + i) for i in range(n)])
    pal = orc.generate_uniform_palette(16)
    taps, div = orc.ed_kernel("floyd_steinberg")
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    got = be.error_diffusion(torch.from_numpy(frames).cuda(), P, taps, div, False).cpu().numpy()
    params = {"variant": "floyd_steinberg", "serpentine": "false"}
    for i in range(n):
        _assert_same(got[i], orc.apply_dithering(frames[i], pal, "error_diffusion", params, False), f"frame {i} of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("perceptual", {}), ("hybrid", {"lum_factor": 1.4, "col_factor": 0.3}),
                                         ("adaptive_variance", {"var_threshold": 200.0, "window_radius": 2}),
                                         ("ostromoukhov", {"serpentine": "false"})])
def test_variable_diffusers_frame_spread_over_workgroups(be, orc, switches, mode, params):
    """The four variable-weight diffusers with few frames in flight and five 64-row bands: a frame's bands run in several
    workgroups (progress words in global memory).  Same bytes as the oracle and as one workgroup per frame."""
    h, w = 290, 130
    arr = orc.rnd(h, w, 21)
    pal = orc.palr(16, 8)
    for gamma in (False, True):
        ref = orc.apply_dithering(arr, pal, mode, params, gamma)
        _assert_same(_run_case(be, orc, arr, pal, mode, params, gamma), ref, f"spread {mode} gamma={gamma}")
    switches.setenv("DP_ED_ONE_WG", "1")
    _assert_same(_run_case(be, orc, arr, pal, mode, params, False), orc.apply_dithering(arr, pal, mode, params, False), f"one workgroup {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,params", [("perceptual", {}), ("hybrid", {"lum_factor": 1.4, "col_factor": 0.3}),
                                         ("adaptive_variance", {"var_threshold": 200.0, "window_radius": 2}),
                                         ("ostromoukhov", {"serpentine": "false"})])
def test_variable_diffusers_persistent_workgroups(be, orc, switches, mode, params):
    """The variable-weight diffusers with several frames per workgroup (DP_ED_GRID: what a batch larger than the number of CUs
    gets): waves run on into the next frame's bands by a running band number.  Every frame against the oracle."""
    import torch
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    h, w, n = 290, 70, 7  # five bands, the last one partial
    frames = np.stack([orc.rnd(h, w, 700 + i) for i in range(n)])
    pal = orc.palr(16, 8)
    switches.setenv("DP_ED_ONE_WG", "1")
    for grid in (1, 3):
        switches.setenv("DP_ED_GRID", str(grid))
        d = ImageDitherer(16, DitherMode(mode), pal, False, params)
        got = d.apply_dithering_frames(torch.from_numpy(frames).cuda()).cpu().numpy()
        for i in range(n):
            _assert_same(got[i], orc.apply_dithering(frames[i], pal, mode, params, False), f"{mode} grid {grid} frame {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("K,seed", [(16, 0), (27, 0), (64, 5), (256, 7)])
def test_diffusers_exact_ties_at_integer_points(be, orc, K, seed):
    """Under the adaptive-variance gate flat regions receive no error: the palette is queried with the pixels themselves,
    and lattice / duplicated palettes tie exactly on many of them.  The kernels answer those from the accelerator's k=1
    tie codes (exact float32 distances, entries in index order) instead of replaying the tree traversal; the result has
    to be scipy's choice.  Content: palette colours, midpoints of palette pairs, lattice midpoints, noise."""
    pal = orc.generate_uniform_palette(K) if seed == 0 else orc.palr(K, seed)
    if K == 64:
        pal = pal[:32] + pal[:32]  # duplicates
    pa = np.asarray(pal, dtype=np.int64)
    rs = np.random.RandomState(K)
    h, w = 96, 150
    i, j = rs.randint(0, len(pal), (2, h, w))
    mid = ((pa[i] + pa[j]) // 2).astype(np.uint8)
    arr = np.where(rs.randint(0, 4, (h, w, 1)) == 0, orc.rnd(h, w, K), mid)
    arr[:8] = pa[i[:8]].astype(np.uint8)
    for mode, params in (("adaptive_variance", {"var_threshold": 1e9, "window_radius": 1}),
                         ("adaptive_variance", {"var_threshold": 900.0, "window_radius": 2}),
                         ("ostromoukhov", {"serpentine": "false"}), ("error_diffusion", {"variant": "floyd_steinberg", "serpentine": "false"})):
        out = _run_case(be, orc, arr, pal, mode, params, False)
        _assert_same(out, orc.apply_dithering(arr, pal, mode, params, False), f"K={K} {mode} {params}")


@pytest.mark.gpu
def test_variance_gate_in_chunks_of_frames(be, orc, switches):
    """The gate pass keeps its two float planes for a chunk of frames only (a gigabyte at most); with a tiny budget a small
    batch already needs several chunks.  Every frame's gate has to equal the scipy restatement's."""
    import torch
    switches.setenv("DP_GATE_CHUNK_BYTES", str(3 * 33 * 47 * 8 + 100))  # three frames per chunk
    frames = np.stack([orc.rnd(33, 47, 50 + i) for i in range(8)])
    pal_f32, oc, lut = orc.prepare_palette(orc.palr(16), False)
    P = be.Palette(pal_f32, oc, lut)
    gates = be.variance_gate(torch.from_numpy(frames).cuda(), P, 250.0, 2).cpu().numpy()
    for i in range(len(frames)):
        ref, _ = orc.variance_gate(frames[i], 250.0, 2)
        assert np.array_equal(gates[i], ref), i


def test_accelerator_built_while_other_threads_launch(be, orc):
    """Host threads sharing one palette (the GUI's preview threads, process_on_devices(devices=[0, 0])): one of them
    crosses the break-even point and builds the accelerator while the others are inside dp_ordered_u8 with the GIL
    dropped.  The library publishes the finished device record whole and launches work on snapshots, so every result is
    right whichever side of the build a launch fell on."""
    import threading
    import torch
    pal = orc.palr(256)
    arr = orc.rnd(270, 480, 3)
    ref = orc.apply_dithering(arr, pal, "bayer", {"size": "8x8"})
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("8x8"))
    for rep in range(3):
        P = be.Palette(*orc.prepare_palette(pal, False))
        P.accel_break_even_pixels = lambda: 6 * 270 * 480   # the build lands in the middle of the launches below
        x = torch.from_numpy(arr).cuda()
        errs = []

        def work():
            try:
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    for _ in range(8):
                        out = be.ordered(x, P, be.MODE_MATRIX, thr=thr)
                        if not np.array_equal(out.cpu().numpy(), ref):
                            errs.append("mismatch")
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        ts = [threading.Thread(target=work) for _ in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert P._accel_done and P.accel_entries > 0
