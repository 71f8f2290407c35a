"""GPU tier: stream discipline of every entry point that takes a `void *stream` (include/*.h: "All work is enqueued
asynchronously on it; the caller synchronises"), on the stalled side stream of tests/streams.py.

Every case runs on a fresh non-blocking stream: a warm run, variant A (the inputs still hold a decoy when the call is
enqueued behind a stall; a part of the call that went to another stream ran early, on the decoy) and variant B (the default
stream is stalled; a part of the call that went to stream 0 ran late, and nothing in the call may wait for it).  The
reference bytes come from the CPU statements of the suite (the oracle, *_ref.py, the library's host statements).  The
backend.* wrapper is the call wherever one exists, so _stream(), _Launch and the per-stream workspace are under test too;
ctypes only where the wrapper uploads host arrays (which waits for the stream) or does not exist.

The controls at the end prove that the harness can fail; if they do not fail on a machine, nothing else here counts.
tests/test_streams_cpu.py checks COVERAGE against the headers.  No test here is meant to fault or hang.

Measured on one MI355X (the full file, 133 cases, 24 s; test_zz_report prints it): the smallest slack, relative to its stall,
was 91.9 ms of T = 121.9 ms (0.75 T: dp_error_diffusion_u8 with 40 colours on (2, 3, 5001), variant B, whose call itself takes
30 ms); no case kept less, and the short ones keep 19.8 of 20 ms; so the factor 4 stands (the rule asks for more than T / 4).
The largest t_warm was 113.6 ms (the first torch op of the session, in the control) and 108.5 ms for a library call (the first
dp_ordered_u8 of the session, which loads the code object); warm runs of later cases take 0.1 to 40 ms."""
import ctypes as C
import zlib

import numpy as np
import pytest

import streams as st

pytestmark = pytest.mark.gpu

# entry point -> the tests below that run it on the stalled stream (tests/test_streams_cpu.py checks this table against the headers)
COVERAGE = {
    "dp_ordered_u8": ["test_ordered", "test_cold_ordered_builds_its_accelerator", "test_two_streams_ordered"],
    "dp_metric_ordered_u8": ["test_metric_ordered", "test_cold_table_modes"],
    "dp_error_diffusion_u8": ["test_error_diffusion", "test_error_diffusion_persistent_grid", "test_cold_diffusion", "test_hand_over"],
    "dp_error_diffusion_numba_u8": ["test_numba_arithmetic"],
    "dp_hybrid_numba_u8": ["test_numba_arithmetic"],
    "dp_variable_diffusion_u8": ["test_variable_diffusion", "test_variable_diffusion_persistent_grid", "test_cold_diffusion"],
    "dp_variance_gate_u8": ["test_variance_gate"],
    "dp_riemersma_u8": ["test_riemersma"],
    "dp_resize_nearest_u8": ["test_resize_nearest"],
    "dp_ign_thresholds": ["test_ign_thresholds"],
    "dp_halftone_pow_flags": ["test_halftone_pow_flags"],
    "dp_halftone_u8": ["test_halftone"],
    "dp_wavelet_u8": ["test_wavelet"],
    "dp_pattern_u8": ["test_pattern", "test_cold_table_modes"],
    "dp_dotdiff_u8": ["test_dotdiff", "test_cold_table_modes"],
    "dp_idiff_u8": ["test_idiff", "test_cold_table_modes"],
    "dp_cells_u8": ["test_cells"],
    "dp_kmeans_step_u8": ["test_kmeans_step", "test_kmeans_step_cell_lists", "test_two_streams_kmeans_cell_lists"],
    "dp_kmeans_hist_build_u8": ["test_kmeans_hist_build"],
    "dp_kmeans_hist_step": ["test_kmeans_hist_step_and_fit"],
    "dp_kmeans_hist_iterate": ["test_kmeans_hist_step_and_fit"],
    "dp_kmeans_update": ["test_kmeans_hist_step_and_fit"],
    "dp_kmeans_plusplus_u8": ["test_kmeans_plusplus"],
    "dp_distinct_first_u8": ["test_distinct_first"],
    "dp_hist_sample_u8": ["test_hist_sample"],
    "dp_distinct_stream_reset": ["test_distinct_stream"],
    "dp_distinct_stream_add_u8": ["test_distinct_stream"],
    "dp_frame_signatures_u8": ["test_scene_signatures_and_distances"],
    "dp_signature_distances": ["test_scene_signatures_and_distances"],
    "dp_index_delta_u8": ["test_index_delta"],
    "dp_gif_lzw_encode_u8": ["test_gif_lzw"],
    "dp_index_from_rgb_u8": ["test_indexed"],
    "dp_rgb_from_index_u8": ["test_indexed"],
    "dp_resize_nearest_plane_u8": ["test_indexed"],
    "dp_png_deflate_encode_u8": ["test_png_deflate"],
    "dp_png_deflate_dyn_encode_u8": ["test_png_deflate"],
    "dp_png_code_lengths_u8": ["test_png_code_lengths"],
    "dp_png_crc32_u8": ["test_png_crc32_and_file"],
    "dp_png_file_assemble_u8": ["test_png_crc32_and_file"],
    "dp_metric_lab_u8": ["test_metric_lab"],
    "dp_okfit_hist_count": ["test_okfit"],
    "dp_okfit_hist_points": ["test_okfit"],
    "dp_okfit_points_u32": ["test_okfit"],
    "dp_okfit_fit": ["test_okfit"],
    "dp_void_cluster_u16": ["test_void_cluster_ranks"],
    "dp_thresholds_blue_noise": ["test_threshold_constructors"],
    "dp_thresholds_void_cluster": ["test_threshold_constructors"],
}
EXCLUDED = {}   # (no entry point with a stream parameter is left out)

DP_OK = 0
KEEP = []       # device objects made inside a stalled run: destroying one frees device memory, which waits for the whole device


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    KEEP.clear()
    torch.cuda.empty_cache()


def _frames(orc, n, h, w, seed):
    return np.stack([orc.rnd(h, w, seed + i) for i in range(n)])


def _per_frame(frames, fn):
    return np.stack([fn(f) for f in frames])


def _frames_data(frames, ref_fn):
    """inputs, ref, decoy_ref of an operation on independent frames.  The decoy of a batch is the batch in reverse order (its
    reference is the reversed reference); that of one frame is the frame turned by 180 degrees, through ref_fn again."""
    want = ref_fn(frames)
    if frames.shape[0] > 1:
        decoy, dwant = np.ascontiguousarray(frames[::-1]), np.ascontiguousarray(want[::-1])
    else:
        decoy = np.ascontiguousarray(frames[:, ::-1, ::-1])
        dwant = ref_fn(decoy)
    return {"in": (frames, decoy)}, {"out": want}, {"out": dwant}


def _run_frames(entry, data, fn, label="", extra=None, **kw):
    """fn(frames tensor, out tensor, state, inp): a frames -> frames call with a caller-supplied output."""
    import torch
    inputs, ref, dref = data
    if extra:
        inputs = dict(inputs, **extra)

    def call(inp, outs, state):
        fn(inp["in"], outs["out"], state, inp)
        return {"out": outs["out"]}

    return st.run_case(st.Case(entry, inputs, ref, call, decoy_ref=dref, outs={"out": (ref["out"].shape, torch.uint8)}, label=label, **kw))


def _tie_rich(orc, pal, n, h, w, seed):
    """Random frames in which every third pixel is a midpoint of two palette entries: the ordered kernels' dirty queue is not
    empty and their second pass runs (as in tests/test_gpu_memory_discipline.py)."""
    frames = _frames(orc, n, h, w, seed)
    pa = np.asarray(pal, np.int64)
    pick = np.random.RandomState(seed).randint(0, len(pal), (n, h, w))
    mid = ((pa[pick] + pa[(pick + 1) % len(pal)]) // 2).astype(np.uint8)
    return np.where(np.random.RandomState(seed + 1).randint(0, 3, (n, h, w, 1)) == 0, mid, frames)


# ================================================================================================ ordered / nearest
ORD_MODES = [("none", {}), ("bayer", {"size": "4x4"}), ("IGN", {"scale": 1.7, "seed": 23})]


def _ordered_call(be, P, thr, mode, params, y0, x0):
    m = {"none": be.MODE_NEAREST, "bayer": be.MODE_MATRIX, "IGN": be.MODE_IGN}[mode]

    def fn(f, out, state, inp):
        be.ordered(f, P, m, thr=thr if m == be.MODE_MATRIX else None, ign_scale=float(params.get("scale", 1.0)),
                   ign_seed=int(params.get("seed", 0)), y0=y0, x0=x0, out=out)
    return fn


@pytest.mark.parametrize("family", ["brute16", "lean256", "compact64", "compactfloat256", "lean300"])
def test_ordered(gpu, orc, family):
    """The families of _ordered_family, the three modes, 4-byte aligned frames of (2, 37, 53) and (1, 3, 1003), tie-rich."""
    from test_gpu_memory_discipline import _ordered_family
    L, be = gpu
    pal, gamma, accel, _ = _ordered_family(orc, family)
    P = be.Palette(*orc.prepare_palette(pal, gamma), accel=accel)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    for i, (n, h, w) in enumerate([(2, 37, 53), (1, 3, 1003)]):
        for j, (mode, params) in enumerate(ORD_MODES):
            y0, x0 = ((0, 0), (5, 3))[(i + j) % 2]
            frames = _tie_rich(orc, pal, n, h, w, 10 * i + j)
            data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.apply_dithering(f, pal, mode, params, gamma, y0=y0, x0=x0)))
            _run_frames("dp_ordered_u8", data, _ordered_call(be, P, thr, mode, params, y0, x0), f"{family} {mode} {(n, h, w)}")


@pytest.mark.parametrize("matrix", [None, "4x4"], ids=["nearest", "bayer"])
def test_metric_ordered(gpu, orc, matrix):
    import metric_ref as mr
    L, be = gpu
    rs = np.random.RandomState(3)
    pal = rs.randint(0, 256, (16, 3)).astype(np.float32)
    outc = rs.randint(0, 256, (16, 3)).astype(np.uint8)
    thr = None if matrix is None else np.ascontiguousarray(orc.bayer_matrix(matrix), np.float32)
    P = be.Palette(pal, outc, metric="oklab")
    T = None if thr is None else be.Thresholds.from_matrix(thr)
    frames = _frames(orc, 2, 37, 53, 7)
    data = _frames_data(frames, lambda fr: mr.ordered_u8(fr, pal, outc, thr, 2, 5))
    _run_frames("dp_metric_ordered_u8", data, lambda f, out, s, inp: be.ordered(f, P, be.MODE_NEAREST if T is None else be.MODE_MATRIX, thr=T, y0=2, x0=5, out=out),
                str(matrix))


# ================================================================================================ error diffusion
# (n, h, w), what: the one-workgroup schedule; the spread schedule with its progress words and repair launch (n_bands >= 4,
# w >= 64, 2 n_frames <= CUs); serpentine rows too wide for LDS: the frame-parallel kernel with its rows in the workspace
ED_SHAPES = [((3, 70, 130), False, "one workgroup"), ((1, 256, 64), False, "spread"), ((2, 3, 5001), True, "serpentine, frame-parallel")]


def _ed_data(orc, frames, pal, variant, serp, gamma=False):
    params = {"variant": variant, "serpentine": "true" if serp else "false"}
    return _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.apply_dithering(f, pal, "error_diffusion", params, gamma)))


def _ed_call(be, orc, P, variant, serp, arithmetic="python"):
    taps, div = orc.ed_kernel(variant)
    return lambda f, out, s, inp: be.error_diffusion(f, P, taps, div, serpentine=serp, out=out, arithmetic=arithmetic)


@pytest.mark.parametrize("K", [16, 40])
def test_error_diffusion(gpu, orc, K):
    L, be = gpu
    pal = orc.generate_uniform_palette(16) if K == 16 else orc.palr(40, 9)
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    for i, ((n, h, w), serp, what) in enumerate(ED_SHAPES):
        variant = "sierra" if serp else "floyd_steinberg"
        data = _ed_data(orc, _frames(orc, n, h, w, 300 + i), pal, variant, serp)
        _run_frames("dp_error_diffusion_u8", data, _ed_call(be, orc, P, variant, serp), f"K={K} {what}")


def test_error_diffusion_persistent_grid(gpu, orc, switches):
    """More frames than workgroups (DP_ED_GRID, the experiments build): waves run on into the next frame's bands."""
    from dither_pie_amd import backend as be
    switches.setenv("DP_ED_ONE_WG", "1")
    switches.setenv("DP_ED_GRID", "2")
    pal = orc.generate_uniform_palette(16)
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    data = _ed_data(orc, _frames(orc, 5, 133, 23, 340), pal, "floyd_steinberg", False)
    _run_frames("dp_error_diffusion_u8", data, _ed_call(be, orc, P, "floyd_steinberg", False), "persistent grid")


def test_numba_arithmetic(gpu, orc):
    L, be = gpu
    pal = orc.palr(16, 3)
    pal_f32, oc, lut = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, oc, lut)
    for i, ((n, h, w), serp, what) in enumerate(ED_SHAPES):
        variant = "jjn" if i % 2 else "floyd_steinberg"
        frames = _frames(orc, n, h, w, 400 + i)
        data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.error_diffusion_numba_u8(f, pal_f32, oc, lut, variant, serp)))
        _run_frames("dp_error_diffusion_numba_u8", data, _ed_call(be, orc, P, variant, serp, "numba"), what)
        if not serp:
            data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.hybrid_numba_u8(f, pal_f32, oc, lut, 1.4, 0.3)))
            _run_frames("dp_hybrid_numba_u8", data, lambda f, out, s, inp: be.hybrid_numba(f, P, 1.4, 0.3, out=out), what)


# ================================================================================================ variable diffusers, gate
def _var_case(be, orc, frames, pal, mode, params, model, serp, label):
    import torch
    gamma = False
    pal_f32, oc, lut = orc.prepare_palette(pal, gamma)
    P = be.Palette(pal_f32, oc, lut, accel=True)
    inputs, ref, dref = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.apply_dithering(f, pal, mode, params, gamma)))
    if model == 3:    # the gate map is an input of the call: it has a decoy too
        inputs["gate"] = tuple(_per_frame(fr, lambda f: orc.variance_gate(f, params["var_threshold"], params["window_radius"])[0]) for fr in inputs["in"])
    if model == 4:
        coef = np.ascontiguousarray(orc.ostromoukhov_coefficients(), np.float32)
        inputs["coef"] = (coef, coef.copy())

    def fn(f, out, s, inp):
        be.variable_diffusion(f, P, model, float(params.get("lum_factor", 0.0)), float(params.get("col_factor", 0.0)), serpentine=serp,
                              gate=inp.get("gate"), coef=inp.get("coef"), out=out)

    _run_frames("dp_variable_diffusion_u8", (inputs, ref, dref), fn, label)


def test_variable_diffusion(gpu, orc):
    """The four diffusers (and Ostromoukhov's serpentine scan): one workgroup per frame and the spread schedule."""
    from test_gpu_memory_discipline import VAR_MODES
    L, be = gpu
    for i, (mode, params, model, serp) in enumerate(VAR_MODES):
        for (n, h, w), what in (((3, 70, 130), "one workgroup"), ((1, 256, 64), "spread")):
            _var_case(be, orc, _frames(orc, n, h, w, 500 + i), orc.palr(16, 8), mode, params, model, serp, f"{mode} serp={serp} {what}")


def test_variable_diffusion_persistent_grid(gpu, orc, switches):
    from dither_pie_amd import backend as be
    from test_gpu_memory_discipline import VAR_MODES
    switches.setenv("DP_ED_ONE_WG", "1")
    switches.setenv("DP_ED_GRID", "2")
    for i, (mode, params, model, serp) in enumerate(VAR_MODES[:4]):
        _var_case(be, orc, _frames(orc, 5, 133, 23, 560 + i), orc.palr(16, 8), mode, params, model, serp, f"{mode} persistent grid")


def test_variance_gate(gpu, orc):
    """The fused path (radius <= 4) and the two-pass path with its float planes in the workspace (radius 5)."""
    L, be = gpu
    for radius, thr, gamma in ((1, 300.0, False), (5, 60.0, True)):
        pal_f32, oc, lut = orc.prepare_palette(orc.palr(16), gamma)
        P = be.Palette(pal_f32, oc, lut)
        frames = np.stack([orc.imgl(37, 53, radius), orc.rnd(37, 53, 600 + radius), orc.imgl(37, 53, radius + 1)])   # smooth and noisy: the gate varies
        frames[2, :20, :30] = 90
        inputs, ref, dref = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.variance_gate(lut[f] if lut is not None else f, thr, radius)[0]))
        st.run_case(st.Case("dp_variance_gate_u8", inputs, ref, lambda inp, outs, s: {"out": be.variance_gate(inp["in"], P, thr, radius)}, decoy_ref=dref,
                            label=f"radius {radius}"))


# ================================================================================================ small per-frame calls
def test_riemersma(gpu, orc):
    import riemersma_ref
    L, be = gpu
    pal = orc.palr(16, 16)
    P = be.Palette(*orc.prepare_palette(pal, False))
    data = _frames_data(_frames(orc, 3, 37, 53, 700), lambda fr: _per_frame(fr, lambda f: riemersma_ref.apply(f, pal, False)))
    _run_frames("dp_riemersma_u8", data, lambda f, out, s, inp: be.riemersma(f, P, out=out))


def test_resize_nearest(gpu, orc):
    from PIL import Image
    L, be = gpu
    oh, ow = 50, 31
    inputs, ref, dref = _frames_data(_frames(orc, 3, 37, 53, 1000),
                                     lambda fr: _per_frame(fr, lambda f: np.array(Image.fromarray(f).resize((ow, oh), Image.NEAREST)).reshape(oh, ow, 3)))
    st.run_case(st.Case("dp_resize_nearest_u8", inputs, ref, lambda inp, outs, s: {"out": be.resize_nearest(inp["in"], oh, ow)}, decoy_ref=dref))


def test_ign_thresholds(gpu, orc):
    """No device input: variant A has nothing to arrive late; variant B sees a launch that went to stream 0."""
    L, be = gpu
    want = np.ascontiguousarray(orc.ign_thresholds(37, 53, 1.7, 23, 11, 2), np.float32)
    st.run_case(st.Case("dp_ign_thresholds", {}, {"out": want}, lambda inp, outs, s: {"out": be.ign_thresholds(37, 53, 1.7, 23, 11, 2)}))


def test_halftone_pow_flags(gpu, orc):
    """Through ctypes (the wrapper, halftone_fixups, reads the count back and caches the list).  The list has no CPU statement
    of its own; what is known of it without the device: the count is in 1 .. cap and was written by this call (the count
    memset and the kernel ran in order), the entries are distinct pixels of the frame, and POW_PIXEL is one of them
    (tests/test_gpu_halftone.py)."""
    import torch
    from test_gpu_memory_discipline import POW_H, POW_PARAMS, POW_PIXEL, POW_W
    L, be = gpu
    hp = be.halftone_params(np.zeros((2, 3), np.float32), **POW_PARAMS)
    cap = 4096

    def call(inp, outs, s):
        assert L.dp_halftone_pow_flags(POW_H, POW_W, C.byref(hp), outs["idx"].data_ptr(), cap, outs["count"].data_ptr(), be._stream()) == DP_OK
        return dict(outs)

    def norm(got):
        c = int(got["count"].view(np.uint64)[0])
        ids = got["idx"][:min(c, cap)] if 0 <= c <= cap else got["idx"][:0]
        return {"facts": np.array([1 <= c <= cap, len(set(ids.tolist())) == len(ids) and bool(((ids >= 0) & (ids < POW_H * POW_W)).all()),
                                   POW_PIXEL in ids.tolist()])}

    st.run_case(st.Case("dp_halftone_pow_flags", {}, {"facts": np.array([True, True, True])}, call, norm=norm,
                        outs={"idx": ((cap,), torch.int32), "count": ((1,), torch.int64)}))


def test_halftone(gpu, orc):
    """Two frames and a palette with duplicated entries: exact ties, so the tie kernel and its count memset run."""
    import halftone_ref
    L, be = gpu
    pal = orc.palr(64, 5)
    pal = pal[:32] + pal[:32]
    P = be.Palette(*orc.prepare_palette(pal, False))
    for params in (dict(dot_gain=1.0, shape="circle"), dict(dot_gain=2.0, shape="square", cell_size=3)):
        full = dict(halftone_ref.DEFAULTS, **params)
        frames = _frames(orc, 2, 37, 53, 800)
        frames[-1] = orc.imgl(37, 53, 3)
        data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: halftone_ref.apply(f, pal, False, **full)))
        _run_frames("dp_halftone_u8", data, lambda f, out, s, inp: be.halftone(f, P, full, out=out), str(params))


def test_wavelet(gpu, orc):
    """Three frames, one of them with a flat channel: the per-frame head memsets."""
    import json
    import os
    import wavelet_ref as wr
    from conftest import GOLDEN
    L, be = gpu
    with open(os.path.join(GOLDEN, "wavelet.json")) as fh:
        taps = json.load(fh)["taps"]
    pal = orc.palr(16, 9)
    P = be.Palette(*orc.prepare_palette(pal, False))
    frames = _frames(orc, 3, 37, 53, 900)
    frames[0, ..., 1] = 77
    params = dict(wavelet="db2", subband_quant=8, seed=42)
    data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: wr.apply(f, pal, False, taps, **params)))
    _run_frames("dp_wavelet_u8", data, lambda f, out, s, inp: be.wavelet(f, P, params, out=out))


# ================================================================================================ table modes
def _table_palette(be, k, seed, gamma=False, metric="rgb"):
    from dither_pie_amd.dithering_lib import prepare_palette
    rs = np.random.RandomState(seed)
    pal_f32, outc, lut = prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], gamma)
    return (pal_f32, outc, lut), (lambda: be.Palette(pal_f32, outc, lut) if metric == "rgb" else be.Palette(pal_f32, outc, metric=metric))


def _pattern_bits(be, orc, shape=(2, 70, 130)):
    import pattern_ref as pr
    (pal_f32, outc, lut), make = _table_palette(be, 16, 50)
    data = _frames_data(_frames(orc, *shape, 50), lambda fr: pr.pattern_frames(orc, fr, pal_f32, outc, lut, 4, 128, y0=1, x0=3))
    return data, make, lambda f, out, P, inp: be.pattern(f, P, 4, 128, y0=1, x0=3, out=out)


def _dotdiff_bits(be, orc, shape=(2, 70, 130)):
    import dotdiff_ref as dr
    (pal_f32, outc, lut), make = _table_palette(be, 16, 60)
    M = np.ascontiguousarray(dr.KNUTH, np.uint8)
    data = _frames_data(_frames(orc, *shape, 60), lambda fr: dr.dotdiff_frames(orc, fr, pal_f32, outc, lut, M, 256))
    return data, make, lambda f, out, P, inp: be.dotdiff(f, P, M, 256, out=out)


def _idiff_bits(be, orc, shape=(2, 70, 130), name="floyd_steinberg"):
    import idiff_ref as ir
    (pal_f32, outc, lut), make = _table_palette(be, 16, 70)
    taps, divisor = ir.KERNELS[name]
    data = _frames_data(_frames(orc, *shape, 70), lambda fr: ir.idiff_frames(orc, fr, pal_f32, outc, lut, taps, divisor, 256))
    return data, make, lambda f, out, P, inp: be.idiff(f, P, taps, divisor, 256, out=out)


def _metric_bits(be, orc, shape=(2, 37, 53)):
    import metric_ref as mr
    rs = np.random.RandomState(4)
    pal, outc = rs.randint(0, 256, (16, 3)).astype(np.float32), rs.randint(0, 256, (16, 3)).astype(np.uint8)
    thr = np.ascontiguousarray(orc.bayer_matrix("4x4"), np.float32)
    T = be.Thresholds.from_matrix(thr)
    data = _frames_data(_frames(orc, *shape, 80), lambda fr: mr.ordered_u8(fr, pal, outc, thr, 0, 0))
    return data, (lambda: be.Palette(pal, outc, metric="oklab")), lambda f, out, P, inp: be.ordered(f, P, be.MODE_MATRIX, thr=T, out=out)


def _warm_table_case(entry, bits, label=""):
    data, make, fn = bits
    P = make()
    return _run_frames(entry, data, lambda f, out, s, inp: fn(f, out, P, inp), label)


def test_pattern(gpu, orc):
    L, be = gpu
    _warm_table_case("dp_pattern_u8", _pattern_bits(be, orc))


def test_dotdiff(gpu, orc):
    L, be = gpu
    _warm_table_case("dp_dotdiff_u8", _dotdiff_bits(be, orc))


def test_idiff(gpu, orc):
    """(2, 70, 130), and (1, 130, 70): one frame whose bands meet through the workspace."""
    L, be = gpu
    _warm_table_case("dp_idiff_u8", _idiff_bits(be, orc))
    _warm_table_case("dp_idiff_u8", _idiff_bits(be, orc, (1, 130, 70), "jjn"), "bands")


def test_cells(gpu, orc):
    import cells_ref as cr
    import torch
    L, be = gpu
    (pal_f32, outc, lut), make = _table_palette(be, 16, 160)
    P = make()
    frames = _frames(orc, 2, 70, 130, 160)
    want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, 8, 8, 2, 0, [0xFFFF], 4, 64)
    inputs = {"in": (frames, np.ascontiguousarray(frames[::-1]))}
    ref = {"out": want, "sets": want_sets}
    dref = {"out": np.ascontiguousarray(want[::-1]), "sets": np.ascontiguousarray(want_sets[::-1])}

    def call(inp, outs, s):
        out, sets = be.cells(inp["in"], P, (8, 8), 2, 4, 64, out=outs["out"], sets=outs["sets"])
        return {"out": out, "sets": sets}

    st.run_case(st.Case("dp_cells_u8", inputs, ref, call, decoy_ref=dref, outs={"out": (frames.shape, torch.uint8), "sets": (want_sets.shape, torch.uint16)}))


# ================================================================================================ k-means, distinct colours
def _km_data(orc, n, K, seed):
    rs = np.random.RandomState(seed)
    px = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    dpx = np.ascontiguousarray(px[::-1] // 2 * 2)
    centers = np.ascontiguousarray(px[rs.randint(0, n, K)].astype(np.float64) + 0.25)
    mean = np.ascontiguousarray(orc.data_mean(px), np.float64)
    refs = []
    for p in (px, dpx):
        s, c, _ = orc.kmeans_step(p, centers, mean)
        x = p.astype(np.int64)
        refs.append({"sums": np.asarray(s, np.int64), "counts": np.asarray(c, np.int64), "sumsq_total": np.array([(x * x).sum()], np.int64)})
    inputs = {"px": (px, dpx), "centers": (centers, centers.copy()), "mean": (mean, mean.copy())}
    return inputs, refs[0], refs[1]


def _km_norm(got):
    return {"sums": got["sums"], "counts": got["counts"], "sumsq_total": np.array([got["sumsq"].sum()], np.int64)}


def _km_call(be):
    def call(inp, outs, s):
        sums, counts, sumsq = be.kmeans_step(inp["px"], inp["centers"], inp["mean"])
        return {"sums": sums, "counts": counts, "sumsq": sumsq}
    return call


@pytest.mark.parametrize("n, K", [(4099, 8), (20000, 32)])
def test_kmeans_step(gpu, orc, n, K):
    """The default pass: three memsets (sums, counts, squared norms are separate tensors) and the kernel."""
    L, be = gpu
    inputs, ref, dref = _km_data(orc, n, K, n)
    st.run_case(st.Case("dp_kmeans_step_u8", inputs, ref, _km_call(be), decoy_ref=dref, norm=_km_norm, label=f"n={n} K={K}"))


@pytest.mark.parametrize("n, K", [(4099, 8), (20000, 32)])
def test_kmeans_step_cell_lists(gpu, orc, switches, n, K):
    """The cell-list pass (the library takes it from 2^19 pixels; DP_KMEANS_CELLS=1 of the experiments build at any size): the
    list build and the pass, with the library's 64 KB of lists for this (device, stream)."""
    from dither_pie_amd import backend as be
    switches.setenv("DP_KMEANS_CELLS", "1")
    inputs, ref, dref = _km_data(orc, n, K, n + 1)
    st.run_case(st.Case("dp_kmeans_step_u8", inputs, ref, _km_call(be), decoy_ref=dref, norm=_km_norm, label=f"cell lists n={n} K={K}"))


def _hist_table_numpy(px):
    r, g, b = (px[:, i].astype(np.int64) for i in range(3))
    idx = ((r >> 4) << 20) | ((g >> 4) << 16) | ((b >> 4) << 12) | ((r & 15) << 8) | ((g & 15) << 4) | (b & 15)
    return np.bincount(idx, minlength=1 << 24).astype(np.uint32)


def _hist_parts(buf):
    """What of a histogram buffer is specified: the table, the per-cell counts, the number of occupied cells, the sorted list
    of them, the overflow word."""
    table = buf[:1 << 26].view(np.uint32)
    info = buf[1 << 26:].view(np.uint32)
    n_occ = int(info[4096])
    return {"table": table, "cells": info[:4097].copy(), "list": np.sort(info[4097:4097 + min(n_occ, 4096)] & 0xfff), "overflow": info[8193:8194].copy()}


def _hist_want(px):
    table = _hist_table_numpy(px)
    per_cell = table.reshape(4096, 4096).sum(1).astype(np.uint32)
    occ = np.nonzero(per_cell)[0].astype(np.uint32)
    return {"table": table, "cells": np.concatenate([per_cell, np.array([len(occ)], np.uint32)]), "list": occ, "overflow": np.zeros(1, np.uint32)}


def test_kmeans_hist_build(gpu, orc):
    L, be = gpu
    px = orc.imgl(1, 8191, 3).reshape(-1, 3)
    px[::5] = np.random.RandomState(1).randint(0, 256, (len(px[::5]), 3))
    dpx = np.ascontiguousarray(px[::-1] // 2 * 2)
    st.run_case(st.Case("dp_kmeans_hist_build_u8", {"px": (px, dpx)}, _hist_want(px), lambda inp, outs, s: {"hist": be.ColourHistogram(inp["px"]).buf},
                        decoy_ref=_hist_want(dpx), norm=lambda got: _hist_parts(got["hist"])))


def test_kmeans_hist_step_and_fit(gpu, orc):
    """dp_kmeans_hist_step on a resident histogram; then a whole fit enqueued without a synchronisation, once with
    dp_kmeans_hist_iterate and once with dp_kmeans_hist_step + dp_kmeans_update.  The late input is the initial centres."""
    import torch
    L, be = gpu
    n, K = 20011, 8
    px = orc.imgl(1, n, 3).reshape(-1, 3)
    px[::5] = np.random.RandomState(1).randint(0, 256, (len(px[::5]), 3))
    mean_np = np.ascontiguousarray(orc.data_mean(px), np.float64)
    inits = [np.ascontiguousarray(px[np.random.RandomState(seed).choice(n, K, replace=False)].astype(np.float64)) for seed in (2, 3)]
    hist = be.ColourHistogram(torch.from_numpy(px).cuda())
    mean = torch.from_numpy(mean_np).cuda()
    torch.cuda.synchronize()

    steps = [orc.kmeans_step(px, c, mean_np) for c in inits]
    x64 = px.astype(np.int64)
    refs = [{"sums": np.asarray(s, np.int64), "counts": np.asarray(c, np.int64), "sumsq_total": np.array([(x64 * x64).sum()], np.int64)} for s, c, _ in steps]

    def step(inp, outs, s):
        sums, counts, sumsq = hist.step(inp["centers"], mean)
        return {"sums": sums, "counts": counts, "sumsq": sumsq}

    # (the squared norms do not depend on the centres: the sums and counts carry the difference between real and decoy)
    st.run_case(st.Case("dp_kmeans_hist_step", {"centers": (inits[0], inits[1])}, refs[0], step, decoy_ref=refs[1], norm=_km_norm))

    fits = [orc.kmeans_lloyd(px, c) for c in inits]                      # (centres, inertia, iterations)
    launches = max(f[2] for f in fits) + 40

    def fit_ref(f):
        return {"centers": np.asarray(f[0], np.float64), "n_iter": np.array([f[2]], np.int64)}

    def fit_norm(want):
        def norm(got):
            st_, c = got["status"], got["centers"]
            ok = int(st_[0]) in (1, 3) and np.abs(c - want[0]).max() < 1e-9 and abs(st_[2] - want[1]) <= 1e-9 * want[1]
            # within the tolerance of tests/test_gpu_memory_discipline.py the centres count as the reference's
            return {"centers": np.asarray(want[0], np.float64) if ok else c, "n_iter": np.array([int(st_[1])], np.int64)}
        return norm

    for fused in (True, False):
        def fit(inp, outs, s, fused=fused):
            centers = inp["centers"].clone()
            totals = torch.zeros(5 * K, dtype=torch.int64, device="cuda")
            prev = torch.zeros((K, 4), dtype=torch.float64, device="cuda")
            status = torch.zeros(8, dtype=torch.float64, device="cuda")
            ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
            for i in range(launches):
                if fused:
                    hist.iterate(centers, totals, prev, status, ticket, 1e-4, 300, i == 0, mean)
                else:
                    hist.step_into(centers, totals, i == 0, mean)
                    be.kmeans_update(totals, centers, prev, status, 1e-4, 300)
            return {"centers": centers, "status": status}

        st.run_case(st.Case("dp_kmeans_hist_iterate" if fused else "dp_kmeans_update", {"centers": (inits[0], inits[1])}, fit_ref(fits[0]), fit,
                            decoy_ref=fit_ref(fits[1]), norm=fit_norm(fits[0]), label="fit"))


def test_kmeans_plusplus(gpu, orc):
    """Through ctypes: the wrapper uploads the caller's uniforms from host memory, which waits for the stream."""
    import torch
    from dither_pie_amd import kmeans
    L, be = gpu
    n, K = 4099, 8
    n_trials = 2 + int(np.log(K))
    data = []
    for seed in (20, 21):
        sample = np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)
        rs = np.random.RandomState(5)
        first = kmeans.first_center_draw(n, rs)
        uniforms = np.ascontiguousarray(np.stack([rs.uniform(size=n_trials) for _ in range(1, K)]))
        c_ref, ids_ref = kmeans.kmeans_plusplus(sample, K, np.random.RandomState(5), return_indices=True)
        data.append((sample, uniforms, first, {"ids": ids_ref.astype(np.int32), "centers": np.asarray(c_ref, np.float64)}))
    assert data[0][2] == data[1][2]
    first = data[0][2]

    def call(inp, outs, s):
        assert L.dp_kmeans_plusplus_u8(inp["sample"].data_ptr(), n, K, first, inp["uniforms"].data_ptr(), n_trials, outs["ids"].data_ptr(),
                                       outs["centers"].data_ptr(), be._stream()) == DP_OK, L.dp_last_error()
        return dict(outs)

    st.run_case(st.Case("dp_kmeans_plusplus_u8", {"sample": (data[0][0], data[1][0]), "uniforms": (data[0][1], data[1][1])}, data[0][3], call,
                        decoy_ref=data[1][3], outs={"ids": ((K,), torch.int32), "centers": ((K, 3), torch.float64)}))


def _few_colours(seed, n, n_colours=40):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n_colours, 3)).astype(np.uint8)[rs.randint(0, n_colours, n)]


def test_distinct_first(gpu, orc):
    """The wrapper reads the count back: it waits for the stream (kind syncs_stream)."""
    import clip_palette_ref as cr
    L, be = gpu
    px, dpx = _few_colours(30, 4099), _few_colours(31, 4099)
    st.run_case(st.Case("dp_distinct_first_u8", {"px": (px, dpx)}, {"out": cr.distinct_first(px)}, lambda inp, outs, s: {"out": be.distinct_first(inp["px"])},
                        decoy_ref={"out": cr.distinct_first(dpx)}, kind="syncs_stream"))


def test_distinct_stream(gpu, orc):
    """add, add, reset, add on one resident object, nothing read back in between: the count and the list after the second add,
    and after the add that follows the reset."""
    import clip_palette_ref as cr
    L, be = gpu
    bufs = [_few_colours(40 + i, n, 60) for i, n in enumerate((4099, 2049, 4097))]
    dbufs = [_few_colours(50 + i, n, 60) for i, n in enumerate((4099, 2049, 4097))]

    def want(b):
        two, last = cr.distinct_first(np.concatenate(b[:2])), cr.distinct_first(b[2])
        return {"n2": np.array([len(two)], np.int64), "list2": two, "n3": np.array([len(last)], np.int64), "list3": last}

    ref, dref = want(bufs), want(dbufs)
    n2, n3 = len(ref["list2"]), len(ref["list3"])

    def call(inp, outs, d):
        d.add(inp["a"]).add(inp["b"])
        got = {"n2": d.count.clone(), "list2": d.list[:3 * n2].clone()}
        d.reset().add(inp["c"])
        got.update(n3=d.count, list3=d.list[:3 * n3])
        return got

    st.run_case(st.Case("dp_distinct_stream_add_u8", {k: (bufs[i], dbufs[i]) for i, k in enumerate("abc")}, ref, call, decoy_ref=dref,
                        prepare=lambda variant: be.DistinctStream()))


def _built_histograms(be, pxs):
    """Histogram buffers of pixel arrays, built by the library on the default stream and complete: INPUTS of the cases below."""
    import torch
    bufs = [be.ColourHistogram(torch.from_numpy(p).cuda()).buf for p in pxs]
    torch.cuda.synchronize()
    return bufs


def _hist_on(be, buf, n):
    h = be.ColourHistogram.__new__(be.ColourHistogram)
    h.buf, h.n = buf, n
    return h


def test_hist_sample(gpu, orc):
    """The wrapper reads the number of bad ranks back (kind syncs_stream).  The histogram's contents are the late input."""
    import clip_palette_ref as cr
    import torch
    L, be = gpu
    rs = np.random.RandomState(12)
    pxs = [np.concatenate([rs.randint(0, 256, (5000, 3)), np.repeat([[17, 200, 3]], 700, axis=0), rs.randint(32, 48, (3000, 3))]).astype(np.uint8) for _ in range(2)]
    ranks = rs.randint(0, len(pxs[0]), 1000).astype(np.int64)
    real, decoy = _built_histograms(be, pxs)
    wants = [cr.rank_sample(cr.histogram(p), ranks) for p in pxs]
    assert wants[0][1] == 0 and wants[1][1] == 0
    r = torch.from_numpy(ranks).cuda()
    st.run_case(st.Case("dp_hist_sample_u8", {"hist": (real, decoy)}, {"out": wants[0][0]}, lambda inp, outs, s: {"out": _hist_on(be, inp["hist"], len(pxs[0])).sample(r)},
                        decoy_ref={"out": wants[1][0]}, kind="syncs_stream"))


# ================================================================================================ scenes, GIF, indexed, PNG
def test_scene_signatures_and_distances(gpu, orc):
    """dp_frame_signatures_u8 with its zeroing memset; then two batches through a SceneStream, the signature carried."""
    import scene_ref as sr
    L, be = gpu
    rs = np.random.RandomState(30)
    frames = rs.randint(0, 256, (4, 37, 53, 3)).astype(np.uint8)
    frames[0, :, :26] = (15, 16, 240)
    decoy = np.ascontiguousarray(frames[::-1])
    sig = sr.signatures(frames)
    st.run_case(st.Case("dp_frame_signatures_u8", {"in": (frames, decoy)}, {"sig": sig.astype(np.uint32)}, lambda inp, outs, s: {"sig": be.frame_signatures(inp["in"])},
                        decoy_ref={"sig": np.ascontiguousarray(sig[::-1]).astype(np.uint32)}))

    def dist(f):
        d = sr.distances(sr.signatures(f), None).astype(np.int64)
        return {"d1": d[:2], "d2": d[2:]}

    def call(inp, outs, scene):
        return {"d1": scene.add(inp["in"][:2]), "d2": scene.add(inp["in"][2:])}

    st.run_case(st.Case("dp_signature_distances", {"in": (frames, decoy)}, dist(frames), call, decoy_ref=dist(decoy), prepare=lambda variant: be.SceneStream()))


def test_index_delta(gpu, orc):
    """Two batches through a DeltaStream: the changed-count memset, the delta kernel, the carried plane."""
    import gif_ref as gr
    L, be = gpu
    rs = np.random.RandomState(40)
    planes = rs.randint(0, 6, (4, 37, 53)).astype(np.uint8)
    planes[2] = planes[1]
    decoy = rs.randint(0, 6, (4, 37, 53)).astype(np.uint8)

    def want(p):
        out, counts = gr.index_delta(p, 200, None)
        return {"o1": out[:2], "c1": np.asarray(counts[:2], np.int64), "o2": out[2:], "c2": np.asarray(counts[2:], np.int64)}

    def call(inp, outs, ds):
        o1, c1 = ds.add(inp["in"][:2], 200)
        o2, c2 = ds.add(inp["in"][2:], 200)
        return {"o1": o1, "c1": c1, "o2": o2, "c2": c2}

    st.run_case(st.Case("dp_index_delta_u8", {"in": (planes, decoy)}, want(planes), call, decoy_ref=want(decoy), prepare=lambda variant: be.DeltaStream()))


def _runs(got, payload="payload", sizes="sizes"):
    """payload [N, stride] and sizes [N] -> the sizes and the specified bytes (the bytes past a size are not)."""
    p, z = got[payload], got[sizes].astype(np.int64)
    return {"sizes": z, "data": np.concatenate([p[f, :int(np.clip(z[f], 0, p.shape[1]))] for f in range(len(z))] + [np.zeros(0, np.uint8)])}


def _runs_want(streams):
    return {"sizes": np.array([len(b) for b in streams], np.int64), "data": np.frombuffer(b"".join(streams), np.uint8)}


def test_gif_lzw(gpu, orc):
    import gif_ref as gr
    L, be = gpu
    rs = np.random.RandomState(50)
    planes, decoy = gr.content("tile", rs, 3, 37, 53, 16), gr.content("noise", rs, 3, 37, 53, 16)
    mcs = max(2, gr.table_bits(16))

    def want(p):
        return _runs_want([gr.image_data(f.reshape(-1), mcs, 700) for f in p])

    def call(inp, outs, s):
        payload, sizes = be.gif_lzw(inp["in"], mcs, chunk_px=700)
        return {"payload": payload, "sizes": sizes}

    st.run_case(st.Case("dp_gif_lzw_encode_u8", {"in": (planes, decoy)}, want(planes), call, decoy_ref=want(decoy), norm=_runs))


def test_indexed(gpu, orc):
    import indexed_ref as ir
    L, be = gpu
    rs = np.random.RandomState(100)
    colours = rs.randint(0, 256, (40, 3)).astype(np.uint8)
    colours[20] = colours[0]
    imap = be.IndexMap(colours)
    rgbs = [colours[rs.randint(0, 40, (3, 37, 53))] for _ in range(2)]
    for r in rgbs:
        r[rs.randint(0, 5, (3, 37, 53)) == 0] = (1, 2, 3)                # a foreign colour: counted

    def to_want(rgb):
        idx, _, n_missing = ir.to_indices(rgb.reshape(-1, 3), colours)
        return {"planes": idx.astype(np.uint8), "count": np.array([n_missing], np.int64)}

    def to_call(inp, outs, s):
        planes, count = be.to_indices(inp["in"], imap, strict=False)
        return {"planes": planes, "count": count}

    st.run_case(st.Case("dp_index_from_rgb_u8", {"in": (rgbs[0], rgbs[1])}, to_want(rgbs[0]), to_call, decoy_ref=to_want(rgbs[1])))

    idxs = [rs.randint(0, 50, (3, 37, 53)).astype(np.uint8) for _ in range(2)]   # 40 .. 49: outside the map, counted

    def from_want(idx):
        rgb, _, n_bad = ir.from_indices(idx.reshape(-1), colours)
        return {"rgb": rgb.astype(np.uint8), "count": np.array([n_bad], np.int64)}

    def from_call(inp, outs, s):
        rgb, count = be.from_indices(inp["in"], imap, strict=False)
        return {"rgb": rgb, "count": count}

    st.run_case(st.Case("dp_rgb_from_index_u8", {"in": (idxs[0], idxs[1])}, from_want(idxs[0]), from_call, decoy_ref=from_want(idxs[1])))
    st.run_case(st.Case("dp_resize_nearest_plane_u8", {"in": (idxs[0], idxs[1])}, {"out": ir.resize_nearest_plane(idxs[0], 50, 31)},
                        lambda inp, outs, s: {"out": be.resize_nearest_plane(inp["in"], 50, 31)}, decoy_ref={"out": ir.resize_nearest_plane(idxs[1], 50, 31)}))


@pytest.mark.parametrize("blocks", ["fixed", "dynamic"])
def test_png_deflate(gpu, orc, blocks):
    """Two planes of 64 x 127 at depth 4 with segments of 2048 bytes: several segments a frame."""
    import png_ref as pr
    L, be = gpu
    rs = np.random.RandomState(60)
    planes, decoy = pr.content("photo", rs, 2, 64, 127, 16), pr.content("tile", rs, 2, 64, 127, 16)

    def want(p):
        streams = be.png_deflate_host(p, 4, 2048, blocks=blocks)           # the library's host statement, checked against zlib here
        for f in range(len(p)):
            assert zlib.decompress(streams[f]) == pr.filtered(p[f], 4)
        return _runs_want(streams)

    def call(inp, outs, s):
        payload, sizes = be.png_deflate(inp["in"], 4, 2048, blocks=blocks)
        return {"payload": payload, "sizes": sizes}

    st.run_case(st.Case("dp_png_deflate_dyn_encode_u8" if blocks == "dynamic" else "dp_png_deflate_encode_u8", {"in": (planes, decoy)}, want(planes), call,
                        decoy_ref=want(decoy), norm=_runs))


def test_png_code_lengths(gpu, orc):
    import png_dyn_ref as dr
    L, be = gpu
    rs = np.random.RandomState(70)
    counts = [rs.randint(0, 40, (3, 30)).astype(np.int32) for _ in range(2)]

    def want(c):
        out = be.png_code_lengths_host(c, 15)
        for i in range(len(c)):
            assert out[i].tolist() == dr.code_lengths(c[i].tolist(), 15)
        return {"out": out}

    st.run_case(st.Case("dp_png_code_lengths_u8", {"in": (counts[0], counts[1])}, want(counts[0]), lambda inp, outs, s: {"out": be.png_code_lengths(inp["in"], 15)},
                        decoy_ref=want(counts[1])))


def test_png_crc32_and_file(gpu, orc):
    import png_file_ref as fr
    import torch
    L, be = gpu
    rs = np.random.RandomState(80)
    stride = 37 * 53
    datas = [rs.randint(0, 256, (3, stride)).astype(np.uint8) for _ in range(2)]
    sizes = [stride, 0, 700]
    z = torch.tensor(sizes, dtype=torch.int64, device="cuda")

    def crc_want(d):
        return {"crc": np.array([zlib.crc32(d[r, :k].tobytes()) for r, k in enumerate(sizes)], np.uint32)}

    st.run_case(st.Case("dp_png_crc32_u8", {"in": (datas[0], datas[1])}, crc_want(datas[0]), lambda inp, outs, s: {"crc": be.png_crc32(inp["in"], z)},
                        decoy_ref=crc_want(datas[1])))

    pre = rs.randint(0, 256, 38).astype(np.uint8)
    pre_dev = torch.from_numpy(pre).cuda()                              # (a prefix on the device: a host one would be uploaded, which waits)

    def file_want(d):
        data, offs = fr.assemble([d[f, :k].tobytes() for f, k in enumerate(sizes)], pre.tobytes(), None, 1, 4, 2)
        return {"offsets": np.asarray(offs, np.int64), "data": np.frombuffer(data, np.uint8)}

    def file_call(inp, outs, s):
        out, offsets = be.png_file_assemble(inp["in"], z, pre=pre_dev, n_idat=1, seq0=4, seq_step=2)
        return {"out": out, "offsets": offsets}

    def file_norm(got):
        end = int(np.clip(got["offsets"][-1], 0, got["out"].size))
        return {"offsets": got["offsets"], "data": got["out"][:end]}

    st.run_case(st.Case("dp_png_file_assemble_u8", {"in": (datas[0], datas[1])}, file_want(datas[0]), file_call, decoy_ref=file_want(datas[1]), norm=file_norm))


# ================================================================================================ Oklab metric and fit
def test_metric_lab(gpu, orc):
    import metric_ref as mr
    L, be = gpu
    rgbs = [np.random.RandomState(70 + i).randint(0, 256, (5000, 3)).astype(np.uint8) for i in range(2)]
    st.run_case(st.Case("dp_metric_lab_u8", {"in": (rgbs[0], rgbs[1])}, {"lab": mr.lab(rgbs[0]).astype(np.int32)}, lambda inp, outs, s: {"lab": be.metric_lab(inp["in"])},
                        decoy_ref={"lab": mr.lab(rgbs[1]).astype(np.int32)}))


def test_okfit(gpu, orc):
    """The two histogram scans (their wrappers read the count back), the records from arrays (ctypes: the wrapper uploads host
    arrays) and the fit, which the header says waits for its stream once per pass."""
    import metric_ref as mr
    import okfit_ref as ok
    import torch
    L, be = gpu
    K = 8
    rs = np.random.RandomState(31)
    pxs = []
    for n_px in (3000, 2600):                                            # (different numbers of colours: the count tells them apart)
        px = rs.randint(0, 256, (n_px, 3)).astype(np.uint8)
        px[:900] = px[900:1800] // 64 * 64
        pxs.append(px)
    pts = [ok.points_of(p) for p in pxs]                                  # (codes, counts)

    def records(codes, counts):
        rec = np.zeros(len(codes), be.OKFIT_POINT_DTYPE)
        rec["code"], rec["count"], rec["lab"] = codes, counts, mr.lab(ok.colours_of(codes))
        return rec

    recs = [records(*p) for p in pts]
    real, decoy = _built_histograms(be, pxs)
    assert len(recs[0]) != len(recs[1])
    st.run_case(st.Case("dp_okfit_hist_count", {"hist": (real, decoy)}, {"n": np.array([len(recs[0])], np.int64)},
                        lambda inp, outs, s: {"n": torch.tensor([_hist_on(be, inp["hist"], 3000).n_occupied()], dtype=torch.int64, device="cuda")},
                        decoy_ref={"n": np.array([len(recs[1])], np.int64)}, kind="syncs_stream"))
    st.run_case(st.Case("dp_okfit_hist_points", {"hist": (real, decoy)}, {"pts": recs[0]}, lambda inp, outs, s: {"pts": _hist_on(be, inp["hist"], 3000).points()},
                        decoy_ref={"pts": recs[1]}, kind="syncs_stream"))

    n = min(len(recs[0]), len(recs[1]))
    arrays = [(np.ascontiguousarray(c[:n], np.uint32), np.ascontiguousarray(k[:n], np.uint32)) for c, k in pts]

    def points_call(inp, outs, s):
        assert L.dp_okfit_points_u32(inp["codes"].data_ptr(), inp["counts"].data_ptr(), n, outs["pts"].data_ptr(), be._stream()) == DP_OK, L.dp_last_error()
        return dict(outs)

    st.run_case(st.Case("dp_okfit_points_u32", {"codes": (arrays[0][0], arrays[1][0]), "counts": (arrays[0][1], arrays[1][1])}, {"pts": recs[0][:n]}, points_call,
                        decoy_ref={"pts": recs[1][:n]}, outs={"pts": ((n, be.OKFIT_POINT_BYTES), torch.uint8)}))

    def fit_want(i):
        pal, centres, n_iter, dist = ok.fit_points(arrays[i][0], arrays[i][1], K, 100)
        return {"pal": np.asarray(pal, np.uint8), "centres": np.asarray(centres, np.int32), "scalars": np.array([n_iter, dist], np.int64)}

    def fit_call(inp, outs, s):
        pal, centres, n_iter, dist = be.okfit(inp["pts"], K, 100)
        return {"pal": torch.from_numpy(pal).cuda(), "centres": torch.from_numpy(centres).cuda(),
                "scalars": torch.tensor([n_iter, dist], dtype=torch.int64, device="cuda")}

    st.run_case(st.Case("dp_okfit_fit", {"pts": (recs[0][:n].view(np.uint8).reshape(n, 16), recs[1][:n].view(np.uint8).reshape(n, 16))}, fit_want(0), fit_call,
                        decoy_ref=fit_want(1), kind="syncs_stream"))


# ================================================================================================ void-and-cluster, constructors
def test_void_cluster_ranks(gpu, orc):
    import torch
    import vac_ref as vr
    L, be = gpu
    want = np.stack([vr.ranks(16, 16, seed, 384) for seed in (3, 4)]).astype(np.int16)
    st.run_case(st.Case("dp_void_cluster_u16", {}, {"out": want}, lambda inp, outs, s: {"out": be.void_cluster_ranks(16, 16, [3, 4], 1.5, out=outs["out"])},
                        outs={"out": ((2, 16, 16), torch.int16)}))


@pytest.mark.parametrize("which", ["blue_noise", "void_cluster"])
def test_threshold_constructors(gpu, orc, which):
    """dp_thresholds_blue_noise and dp_thresholds_void_cluster generate on `stream` and wait for it (kind syncs_stream).  The
    matrix is looked at on the device: the frames dithered with it on the same stream must be the oracle's for the statement's
    matrix (reading the matrix back with dp_thresholds_download would itself wait for the default stream)."""
    import vac_ref as vr
    L, be = gpu
    pal = orc.palr(16, 3)
    pal_f32, oc, lut = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, oc, lut)
    if which == "blue_noise":
        matrix = orc.blue_noise(32, 5)
        make = lambda: be.Thresholds.blue_noise(32, 5)                    # noqa: E731
    else:
        matrix = vr.thresholds(vr.ranks(16, 24, 7, 384))
        make = lambda: be.Thresholds.void_cluster(16, 24, 7, 1.5)         # noqa: E731
    matrix = np.ascontiguousarray(matrix, np.float32)
    data = _frames_data(_frames(orc, 2, 37, 53, 90), lambda fr: _per_frame(fr, lambda f: orc.ordered_u8(f, pal_f32, oc, lut, "matrix", thr=matrix)))

    def fn(f, out, s, inp):
        T = make()
        KEEP.append(T)
        be.ordered(f, P, be.MODE_MATRIX, thr=T, out=out)

    _run_frames("dp_thresholds_" + which, data, fn, kind="syncs_stream")


# ================================================================================================ cold cases, hand-over
COLD_T_MS = st.MIN_STALL_MS   # the stall of the matching warm cases (their warm runs take well under 5 ms)


def _cold(entry, bits, label=""):
    """A fresh palette per variant: the first call builds its table.  Only the bytes are asked for."""
    data, make, fn = bits

    def prepare(variant):
        P = make()
        KEEP.append(P)
        return P

    return _run_frames(entry, data, lambda f, out, P, inp: fn(f, out, P, inp), label, kind="cold", T_ms=COLD_T_MS, prepare=prepare)


def test_cold_table_modes(gpu, orc):
    """dp_pattern_u8, dp_dotdiff_u8, dp_idiff_u8 and dp_metric_ordered_u8 build their table at the first call, on the caller's stream."""
    L, be = gpu
    _cold("dp_pattern_u8", _pattern_bits(be, orc, (2, 37, 53)), "cold")
    _cold("dp_dotdiff_u8", _dotdiff_bits(be, orc, (2, 37, 53)), "cold")
    _cold("dp_idiff_u8", _idiff_bits(be, orc, (2, 37, 53)), "cold")
    _cold("dp_metric_ordered_u8", _metric_bits(be, orc), "cold")


def _ed40_bits(be, orc):
    pal = orc.palr(40, 9)
    taps, div = orc.ed_kernel("floyd_steinberg")
    data = _ed_data(orc, _frames(orc, 3, 70, 130, 300), pal, "floyd_steinberg", False)
    return data, (lambda: be.Palette(*orc.prepare_palette(pal, False))), lambda f, out, P, inp: be.error_diffusion(f, P, taps, div, out=out)


def test_cold_diffusion(gpu, orc):
    """dp_error_diffusion_u8 with 40 colours and dp_variable_diffusion_u8 build their candidate tables at the first call, on the
    null stream, and upload them synchronously."""
    L, be = gpu
    _cold("dp_error_diffusion_u8", _ed40_bits(be, orc), "cold K=40")
    pal = orc.palr(40, 8)
    data = _frames_data(_frames(orc, 3, 70, 130, 500), lambda fr: _per_frame(fr, lambda f: orc.apply_dithering(f, pal, "perceptual", {}, False)))
    _cold("dp_variable_diffusion_u8", (data, (lambda: be.Palette(*orc.prepare_palette(pal, False))),
                                      lambda f, out, P, inp: be.variable_diffusion(f, P, be.DIFFUSER_PERCEPTUAL, out=out)), "cold perceptual")


def test_cold_ordered_builds_its_accelerator(gpu, orc):
    """dp_ordered_u8 with the break-even point lowered, as test_accelerator_built_while_other_threads_launch does: the call that
    crosses it builds the accelerator (synchronously, on the null stream) and then launches on the caller's stream."""
    L, be = gpu
    pal = orc.palr(256, 21)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    frames = _tie_rich(orc, pal, 2, 37, 53, 5)
    data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: orc.apply_dithering(f, pal, "bayer", {"size": "4x4"}, False)))

    def make():
        P = be.Palette(*orc.prepare_palette(pal, False))
        P.accel_break_even_pixels = lambda: 1
        return P

    def fn(f, out, P, inp):
        be.ordered(f, P, be.MODE_MATRIX, thr=thr, out=out)
        assert P._accel_done and P.accel_entries > 0

    _cold("dp_ordered_u8", (data, make, fn), "cold accelerator")


def test_hand_over(gpu, orc):
    """A cold call on s1 and, with no synchronisation by the test, an async case of the same palette on a fresh s2: the table the
    first call built must be complete for every stream when that call returns."""
    import torch
    L, be = gpu
    data, make, fn = _ed40_bits(be, orc)
    P = make()
    x = torch.from_numpy(data[0]["in"][0]).cuda()
    out1, out2 = torch.empty_like(x), torch.empty_like(x)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        fn(x, out1, P, None)                                            # cold: builds and publishes the candidate tables
    with torch.cuda.stream(s2):
        fn(x, out2, P, None)                                            # the first use of them on another stream, nothing waited for
    s2.synchronize()
    if not np.array_equal(out2.cpu().numpy(), data[1]["out"]):
        raise st.StreamOrderError("dp_error_diffusion_u8", "hand-over", "bytes", "the call that followed a cold call on another stream")
    s1.synchronize()
    assert np.array_equal(out1.cpu().numpy(), data[1]["out"])
    _run_frames("dp_error_diffusion_u8", data, lambda f, out, s, inp: fn(f, out, P, inp), "after a cold call on another stream")


# ================================================================================================ two streams at once
def _two_streams(entry, enqueue, check):
    """enqueue(i) under stream i of two, both behind a stall and both enqueued before either is synchronised; check(i, result)."""
    import torch
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, s in enumerate(ss):                                           # warm: workspaces and lists of both streams exist
        with torch.cuda.stream(s):
            check(i, enqueue(i), "warm")
    torch.cuda.synchronize()
    got = []
    for i, s in enumerate(ss):
        with torch.cuda.stream(s):
            st.stall(st.MIN_STALL_MS)
            got.append(enqueue(i))
    for i, s in enumerate(ss):
        s.synchronize()
    for i in range(2):
        check(i, got[i], "A")


def test_two_streams_kmeans_cell_lists(gpu, orc, switches):
    """dp_kmeans_step_u8 through the cell-list pass on two streams with different centres: each (device, stream) has its own 64 KB
    of lists, so neither pass may see the other's."""
    import torch
    from dither_pie_amd import backend as be
    switches.setenv("DP_KMEANS_CELLS", "1")
    n, K = 20000, 32
    rs = np.random.RandomState(9)
    px = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    cs = [np.ascontiguousarray(px[rs.randint(0, n, K)].astype(np.float64) + 0.25) for _ in range(2)]
    mean = np.ascontiguousarray(orc.data_mean(px), np.float64)
    refs = [orc.kmeans_step(px, c, mean) for c in cs]
    assert not np.array_equal(refs[0][1], refs[1][1])
    dpx, dmean = torch.from_numpy(px).cuda(), torch.from_numpy(mean).cuda()
    dcs = [torch.from_numpy(c).cuda() for c in cs]
    torch.cuda.synchronize()

    def check(i, got, variant):
        sums, counts, _ = (t.cpu().numpy() for t in got)
        if not (np.array_equal(sums, refs[i][0]) and np.array_equal(counts, refs[i][1])):
            raise st.StreamOrderError("dp_kmeans_step_u8", variant, "bytes", f"the totals of stream {i} are not the reference's")

    _two_streams("dp_kmeans_step_u8", lambda i: be.kmeans_step(dpx, dcs[i], dmean), check)


def test_two_streams_ordered(gpu, orc):
    """dp_ordered_u8 with one shared palette on two streams, each with its own workspace (flag bitmap, dirty queue)."""
    import torch
    L, be = gpu
    pal = orc.palr(256, 21)
    P = be.Palette(*orc.prepare_palette(pal, False), accel=True)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    fr = [_tie_rich(orc, pal, 2, 37, 53, 20 + i) for i in range(2)]
    refs = [_per_frame(f, lambda x: orc.apply_dithering(x, pal, "bayer", {"size": "4x4"}, False)) for f in fr]
    dev = [torch.from_numpy(f).cuda() for f in fr]
    torch.cuda.synchronize()

    def check(i, got, variant):
        if not np.array_equal(got.cpu().numpy(), refs[i]):
            raise st.StreamOrderError("dp_ordered_u8", variant, "bytes", f"the frames of stream {i} are not the reference's")

    _two_streams("dp_ordered_u8", lambda i: be.ordered(dev[i], P, be.MODE_MATRIX, thr=thr), check)


# ================================================================================================ the Python layer
def _layer_cases(orc):
    """name -> (name, DitherMode or strategy factory, dither_params, reference(frame, palette))"""
    import cells_ref as cr
    import dotdiff_ref as dr
    import idiff_ref as ir
    import metric_ref as mr
    import pattern_ref as pr
    import riemersma_ref
    import vac_ref as vr
    from dither_pie_amd import dithering_lib as dl
    M = dl.DitherMode

    def oracle(mode, params):
        return lambda f, pal: orc.apply_dithering(f, pal, mode, params, False)

    def prepared(fn):
        return lambda f, pal: fn(f, *dl.prepare_palette(pal, False))

    cases = [
        ("none", M.NONE, {}, oracle("none", {})),
        ("bayer", M.BAYER, {"size": "4x4"}, oracle("bayer", {"size": "4x4"})),
        ("blue_noise", M.BLUE_NOISE, {"size": 32, "seed": 5}, oracle("blue_noise", {"size": 32, "seed": 5})),
        ("IGN", M.INTERLEAVED_GRADIENT_NOISE, {"scale": 1.7, "seed": 23}, oracle("IGN", {"scale": 1.7, "seed": 23})),
        ("polka_dot", M.POLKA_DOT, {"tile_size": 8, "gamma": 1.5}, oracle("polka_dot", {"tile_size": 8, "gamma": 1.5})),
        ("error_diffusion", M.ERROR_DIFFUSION, {"variant": "floyd_steinberg", "serpentine": "false"},
         oracle("error_diffusion", {"variant": "floyd_steinberg", "serpentine": "false"})),
        ("riemersma", M.RIEMERSMA, {}, lambda f, pal: riemersma_ref.apply(f, pal, False)),
        ("perceptual", M.PERCEPTUAL, {}, oracle("perceptual", {})),
        ("hybrid", M.HYBRID, {"lum_factor": 1.4, "col_factor": 0.3}, oracle("hybrid", {"lum_factor": 1.4, "col_factor": 0.3})),
        ("adaptive_variance", M.ADAPTIVE_VARIANCE, {"var_threshold": 200.0, "window_radius": 2},
         oracle("adaptive_variance", {"var_threshold": 200.0, "window_radius": 2})),
        ("ostromoukhov", M.OSTROMOUKHOV, {"serpentine": "false"}, oracle("ostromoukhov", {"serpentine": "false"})),
        ("pattern", lambda: dl.PatternDitherStrategy("4x4", 0.5), {}, prepared(lambda f, p, o, l: pr.pattern_u8(orc, f, p, o, l, 4, 128))),
        ("dot diffusion", lambda: dl.DotDiffusionDitherStrategy(), {}, prepared(lambda f, p, o, l: dr.dotdiff_u8(orc, f, p, o, l, np.ascontiguousarray(dr.KNUTH, np.uint8), 256))),
        ("cells", lambda: dl.CellPaletteDitherStrategy(), {}, prepared(lambda f, p, o, l: cr.cells_u8(f, p, o, l, 8, 8, 2, 0, [0xFFFF], 4, 64)[0])),
        ("void and cluster", lambda: dl.VoidAndClusterDitherStrategy(16, 7, 1.5), {},
         prepared(lambda f, p, o, l: orc.ordered_u8(f, p, o, l, "matrix", thr=np.ascontiguousarray(vr.thresholds(vr.ranks(16, 16, 7, 384)), np.float32)))),
        ("integer diffusion", lambda: dl.IntegerErrorDiffusionDitherStrategy("floyd_steinberg", 1.0), {},
         prepared(lambda f, p, o, l: ir.idiff_u8(orc, f, p, o, l, *ir.KERNELS["floyd_steinberg"], 256))),
    ]
    return {c[0]: c for c in cases}, mr


LAYER = ["none", "bayer", "blue_noise", "IGN", "polka_dot", "error_diffusion", "riemersma", "perceptual", "hybrid", "adaptive_variance", "ostromoukhov",
         "pattern", "dot diffusion", "cells", "void and cluster", "integer diffusion"]


def _first_use(entry, data, run, label):
    """The first-use-of-everything form: before each variant the palette, threshold and index-map caches are dropped and the
    ditherer is new, so the call creates every device object it needs behind the stall.  Kind cold: the bytes."""
    from dither_pie_amd import dithering_lib as dl

    def prepare(variant):
        dl.drop_device_caches()
        return None

    try:
        return _run_frames(entry, data, lambda f, out, s, inp: run(f, out), label, kind="cold", T_ms=COLD_T_MS, prepare=prepare)
    finally:
        dl.drop_device_caches()


@pytest.mark.parametrize("name", LAYER)
def test_python_layer_modes(gpu, orc, name):
    """ImageDitherer.apply_dithering_frames on (2, 37, 53) for every DitherMode of the backend and the strategy instances."""
    from dither_pie_amd import dithering_lib as dl
    cases, _ = _layer_cases(orc)
    _, mode, params, ref = cases[name]
    pal = orc.palr(16, 3)
    data = _frames_data(_frames(orc, 2, 37, 53, 11), lambda fr: _per_frame(fr, lambda f: ref(f, pal)))

    def run(f, out):
        d = dl.ImageDitherer(16, mode() if callable(mode) else mode, pal, False, params)
        d.apply_dithering_frames(f, out=out)

    _first_use("ImageDitherer.apply_dithering_frames", data, run, name)


def test_python_layer_halftone_wavelet_and_oklab(gpu, orc):
    """Halftone and wavelet through dither_frames, and metric="oklab" with Bayer through the ditherer."""
    import json
    import os
    import halftone_ref
    import metric_ref as mr
    import wavelet_ref as wr
    from conftest import GOLDEN
    from dither_pie_amd import dithering_lib as dl
    pal = orc.palr(16, 3)
    frames = _frames(orc, 2, 37, 53, 12)
    data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: halftone_ref.apply(f, pal, False, **halftone_ref.DEFAULTS)))
    _first_use("HalftoneDitherStrategy.dither_frames", data, lambda f, out: dl.HalftoneDitherStrategy().dither_frames(f, pal, False, out=out), "halftone")
    with open(os.path.join(GOLDEN, "wavelet.json")) as fh:
        taps = json.load(fh)["taps"]
    data = _frames_data(frames, lambda fr: _per_frame(fr, lambda f: wr.apply(f, pal, False, taps, wavelet="haar", subband_quant=8, seed=42)))
    _first_use("WaveletDitherStrategy.dither_frames", data, lambda f, out: dl.WaveletDitherStrategy().dither_frames(f, pal, False, out=out), "wavelet")
    pal_f32, outc, _ = dl.prepare_palette(pal, False)
    thr = np.ascontiguousarray(orc.bayer_matrix("4x4"), np.float32)
    data = _frames_data(frames, lambda fr: mr.ordered_u8(fr, pal_f32, outc, thr, 0, 0))
    _first_use("ImageDitherer.apply_dithering_frames", data,
               lambda f, out: dl.ImageDitherer(16, dl.DitherMode.BAYER, pal, False, {"size": "4x4"}, metric="oklab").apply_dithering_frames(f, out=out), "oklab bayer")


# ================================================================================================ controls
def _control_data():
    x = (np.arange(4096, dtype=np.int64) * 7 % 251).astype(np.uint8)
    d = (np.arange(4096, dtype=np.int64) * 11 % 241).astype(np.uint8)
    return x, d


def _control(call, ref_fn, **kw):
    x, d = _control_data()
    return st.Case("control", {"in": (x, d)}, {"out": ref_fn(x)}, call, decoy_ref={"out": ref_fn(d)}, **kw)


def test_control_a_well_behaved_op_passes(gpu):
    stat = st.run_case(_control(lambda inp, outs, s: {"out": inp["in"] * 2 + 1}, lambda x: x * 2 + 1))
    assert stat["slack_A_ms"] > 0 and stat["slack_B_ms"] > 0 and stat["T_ms"] >= st.MIN_STALL_MS


def test_control_a_first_stage_on_the_default_stream_fails_variant_a(gpu):
    """A two-stage op whose first stage runs on the default stream: it read the decoy."""
    import torch

    def call(inp, outs, s):
        with torch.cuda.stream(torch.cuda.default_stream()):
            half = inp["in"] * 2
        return {"out": half + 1}

    with pytest.raises(st.StreamOrderError) as e:
        st.run_case(_control(call, lambda x: x * 2 + 1), variants=("A",))
    assert (e.value.variant, e.value.condition) == ("A", "bytes")


def test_control_zeroing_on_the_default_stream_fails_variant_b_only(gpu):
    """An accumulate op whose zeroing runs on the default stream: in A the zeroing is merely early (the buffer is the op's
    own); in B it lands after the accumulation and the result is zero."""
    import torch
    acc = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def call(inp, outs, s):
        with torch.cuda.stream(torch.cuda.default_stream()):
            acc.zero_()
        acc.add_(inp["in"])
        return {"out": acc}

    case = _control(call, lambda x: x.copy())
    st.run_case(case, variants=("A",))
    with pytest.raises(st.StreamOrderError) as e:
        st.run_case(case, variants=("B",))
    assert (e.value.variant, e.value.condition) == ("B", "bytes")


def test_control_a_real_kernel_on_the_null_stream_fails_variant_a(gpu, orc):
    """dp_riemersma_u8 through ctypes with stream = NULL while the case runs on the side stream."""
    import riemersma_ref
    L, be = gpu
    pal = orc.palr(16, 16)
    P = be.Palette(*orc.prepare_palette(pal, False))
    n, h, w = 3, 37, 53
    data = _frames_data(_frames(orc, n, h, w, 700), lambda fr: _per_frame(fr, lambda f: riemersma_ref.apply(f, pal, False)))

    def fn(f, out, s, inp):
        assert L.dp_riemersma_u8(f.data_ptr(), out.data_ptr(), n, h, w, P._h, None) == DP_OK

    with pytest.raises(st.StreamOrderError) as e:
        _run_frames("dp_riemersma_u8", data, fn, "stream = NULL")
    assert (e.value.entry, e.value.variant, e.value.condition) == ("dp_riemersma_u8", "A", "bytes")


def test_control_a_device_synchronisation_fails_variant_b_as_waited(gpu):
    import torch

    def call(inp, outs, s):
        out = inp["in"] * 2 + 1
        torch.cuda.synchronize()
        return {"out": out}

    with pytest.raises(st.StreamOrderError) as e:
        st.run_case(_control(call, lambda x: x * 2 + 1), variants=("B",))
    assert (e.value.variant, e.value.condition) == ("B", "waited")


def test_control_a_stall_too_short_is_vacuous(gpu):
    with pytest.raises(st.StreamOrderError) as e:
        st.run_case(_control(lambda inp, outs, s: {"out": inp["in"] * 2 + 1}, lambda x: x * 2 + 1, force_T_ms=0), variants=("A",))
    assert (e.value.variant, e.value.condition) == ("A", "vacuous")


def test_zz_report(gpu):
    """The timing the harness collected in this session (printed; pytest -rP shows it): per case t_warm, T and the slack -- how
    much of the stall was left when E was asked.  Full file on one MI355X: see the module docstring."""
    slack, warm = st.summary()
    print(f"stream discipline: {len(st.STATS)} cases; smallest slack {slack}; largest t_warm {warm}")
    for s in sorted(st.STATS, key=lambda s: -(s["t_warm_ms"] or 0))[:10]:
        print("  ", s)
