"""GPU tier: memory discipline of every device entry point of the C ABI (include/ditherpie_hip.h).

The value tests hand the library exact-size torch tensors (rounded up and 512-byte aligned by the caching allocator) and a
scratch buffer that is larger than asked and holds whatever the last test left.  Here every pointer the library sees lies
inside one guarded arena (tests/arena.py): inputs and outputs of exactly the documented size at odd addresses, a workspace
of EXACTLY *_workspace_bytes() bytes that is 16- but not 32-byte aligned, guards of >= 1 MiB and >= one frame on both
sides of every region.  Each case runs three times -- workspace pre-filled with zeros, with 0xFF (NaN / -1 / UINT_MAX) and
with noise, guards re-seeded -- and asserts DP_OK, the operation's reference output, byte-identical outputs across the
fills, intact guards, untouched inputs; then, where there is a workspace, that `need - 1` bytes are refused with
DP_EWORKSPACE, an error text that names the function, and no launch (outputs still hold their fill).

Out of scope: in == out aliasing (the header does not specify it).  No test here is meant to fault."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import arena as ar
import halftone_ref
import riemersma_ref
import wavelet_ref as wr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# entry point -> the tests below that run it inside the arena (tests/test_arena_cpu.py checks this table against the header)
COVERAGE = {
    "dp_ordered_u8": ["test_ordered_product_kernels", "test_ordered_kernel_families_traced", "test_ordered_forced_tables"],
    "dp_error_diffusion_u8": ["test_error_diffusion", "test_error_diffusion_persistent_grid"],
    "dp_error_diffusion_numba_u8": ["test_numba_arithmetic"],
    "dp_hybrid_numba_u8": ["test_numba_arithmetic"],
    "dp_variable_diffusion_u8": ["test_variable_diffusion", "test_variable_diffusion_persistent_grid"],
    "dp_variance_gate_u8": ["test_variance_gate"],
    "dp_riemersma_u8": ["test_riemersma"],
    "dp_halftone_u8": ["test_halftone"],
    "dp_halftone_pow_flags": ["test_halftone_pow_flags_respects_cap"],
    "dp_wavelet_u8": ["test_wavelet"],
    "dp_resize_nearest_u8": ["test_resize_nearest"],
    "dp_ign_thresholds": ["test_ign_thresholds"],
    "dp_kmeans_step_u8": ["test_kmeans_step"],
    "dp_kmeans_hist_build_u8": ["test_kmeans_histogram_and_fit"],
    "dp_kmeans_hist_step": ["test_kmeans_histogram_and_fit"],
    "dp_kmeans_hist_iterate": ["test_kmeans_histogram_and_fit"],
    "dp_kmeans_update": ["test_kmeans_histogram_and_fit"],
    "dp_kmeans_plusplus_u8": ["test_kmeans_plusplus"],
    "dp_distinct_first_u8": ["test_distinct_first"],
}
EXCLUDED = {}   # (no device entry point is left out; constructors, host-only and profiling calls take no *_dev pointer)

DP_OK, DP_EWORKSPACE = 0, 5
FILLS = ("zeros", "ones", ar.noise(77))
# (in, out) residues mod 16: 0..3, odd values >= 8; every entry point's first case has an odd `in` and an odd `out`
OFFS = [(1, 3), (3, 1), (0, 9), (2, 13), (13, 0), (9, 2), (15, 7), (5, 11)]
# frames x h x w: 1x1, w = 1, a row of 21 bytes (w * 3 % 4 = 1), three frames of 105 bytes (frames 1, 2 at odd addresses)
SHAPES = [(1, 1, 1), (1, 7, 1), (1, 5, 7), (3, 5, 7)]

with open(os.path.join(GOLDEN, "wavelet.json")) as _fh:
    WL_TAPS = json.load(_fh)["taps"]


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _sync():
    import torch
    torch.cuda.synchronize()


def run_op(L, fn, inputs, outputs, ws_need, call, verify, frame_bytes=1, misaligned=False, compare=None, seed=0, refuse=True):
    """The matrix step for one case.  inputs: name -> (array, residue[, align]); outputs: name -> (nbytes, residue[, align]);
    call(p, ws_ptr, ws_bytes) -> rc with p: name -> address (and p["arena"]: the arena, for fake ops); verify(o) with o:
    name -> uint8 bytes of every output; compare(o): the bytes that must not depend on the scratch fill (default: every
    output byte); refuse: also ask for the refusal of a workspace one byte short (and, misaligned, of ws + 8).  The outputs
    are pre-filled too, with another of the three fills than the workspace, so a stale result of the previous run cannot pass."""
    g = ar.guard_bytes(frame_bytes)
    specs = [(np.asarray(v[0]).nbytes, g, v[2] if len(v) > 2 else 16) for v in inputs.values()]
    specs += [(v[0], g, v[2] if len(v) > 2 else 16) for v in outputs.values()]
    if ws_need:
        specs.append((ws_need, g, 16))
    A = ar.Arena(ar.capacity_for(specs), "cuda", seed)
    for name, v in inputs.items():
        A.carve(name, np.asarray(v[0]).nbytes, v[1], g, *v[2:])
        A.put(name, v[0])
    for name, v in outputs.items():
        A.carve(name, v[0], v[1], g, *v[2:])
    ws = 0
    if ws_need:
        A.carve("ws", ws_need, 0, g)
        ws = A.ptr("ws")
        assert ws % 16 == 0 and ws % 32 == 16 and A.view("ws").numel() == ws_need
    p = {name: A.ptr(name) for name in list(inputs) + list(outputs)}
    p["arena"] = A
    out_fills = ("ones", ar.noise(seed * 1000 + 101), "zeros")
    kept = []
    for i, fill in enumerate(FILLS):
        A.reseed(seed * 1000 + 17 * i + 1)
        for name in outputs:
            A.fill(name, out_fills[i])
        if ws_need:
            A.fill("ws", fill)
        rc = call(p, ws, ws_need)
        _sync()
        assert rc == DP_OK, (fn, fill, rc, L.dp_last_error())
        o = {name: A.get(name).copy() for name in outputs}
        verify(o)
        A.check()
        for name in inputs:
            A.unchanged(name)
        kept.append(compare(o) if compare else o)
    for k in kept[1:]:
        for name in kept[0]:
            assert np.array_equal(kept[0][name], k[name]), f"{fn}: '{name}' depends on what the workspace held before the call"
    if ws_need and refuse:
        refusals = [(ws, ws_need - 1)] + ([(ws + 8, ws_need)] if misaligned else [])
        for ws_ptr, ws_bytes in refusals:
            for name in outputs:
                A.fill(name, ar.noise(seed * 1000 + 500))
            A.fill("ws", ar.noise(seed * 1000 + 501))
            rc = call(p, ws_ptr, ws_bytes)
            msg = L.dp_last_error() or b""
            _sync()
            assert rc == DP_EWORKSPACE, (fn, rc, msg)
            assert fn.encode() in msg, (fn, msg)
            for name in outputs:
                A.unchanged(name)                                  # nothing was launched
            A.unchanged("ws")
            A.check()
    del A


def _frames(orc, n, h, w, seed):
    return np.stack([orc.rnd(h, w, seed + i) for i in range(n)])


def _per_frame(frames, fn):
    return np.stack([fn(f) for f in frames])


def _eq(got, want, what):
    got = got.reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ from the reference, first at {bad[0].tolist()}")


# ================================================================================================ ordered / nearest
# launch_ordered admits its table kernels (fast / lean / compact on integer palettes, compact_float / lean_float under
# use_gamma) only when frames and output are 4-byte aligned; any other address takes the whole-table kernel ("cell") or the
# brute-force kernels ("brute").  So every shape and mode runs twice: at residues that are 4-byte aligned and no better
# (4 and 12 mod 16), and at odd ones.  Which family a case reached is checked where it can be: the experiments library names
# the pass-1 kernel of every launch on stderr under DP_ORDERED_TRACE=1 (no other effect), and the product test runs the same
# cases on the library that ships, whose dispatch is the same code.
ORD_OFFS = {True: [(4, 12), (12, 4), (4, 4), (12, 12)], False: OFFS}
FALLBACK = {"cell", "brute"}
ORD_SHAPES = SHAPES + [(2, 37, 53), (1, 3, 1003), (2, 61, 67)]   # ... 8174 pixels: two 4096-pixel tiles, the second partial
ORD_BIG = (1, 601, 1789)                                          # more 4096-pixel tiles than CUs: the persistent grid's tail
MODES = ("none", "bayer", "IGN")


def _ordered_cases(L, be, orc, pal, gamma, accel, shapes, what, seed0, expect=None, capfd=None, big=None):
    """expect: mode -> the family the 4-byte aligned case must reach (checked when capfd is given: the traced library)."""
    import re
    P = be.Palette(*orc.prepare_palette(pal, gamma), accel=accel)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("4x4"))
    modes = [("none", {}, be.MODE_NEAREST), ("bayer", {"size": "4x4"}, be.MODE_MATRIX), ("IGN", {"scale": 1.7, "seed": 23}, be.MODE_IGN)]
    cases = [(shape, aligned) for shape in shapes for aligned in (True, False)] + ([(big, True)] if big else [])
    reached = set()
    i = 0
    for (n, h, w), aligned in cases:
        for mode, params, m in modes:
            y0, x0 = ((0, 0), (5, 3))[i % 2]
            frames = _frames(orc, n, h, w, seed0 + i)
            if h * w > 64:   # tie-rich content: palette colours and midpoints
                pa = np.asarray(pal, np.int64)
                pick = np.random.RandomState(i).randint(0, len(pal), (n, h, w))
                mid = ((pa[pick] + pa[(pick + 1) % len(pal)]) // 2).astype(np.uint8)
                frames = np.where(np.random.RandomState(i + 1).randint(0, 3, (n, h, w, 1)) == 0, mid, frames)
            want = _per_frame(frames, lambda f: orc.apply_dithering(f, pal, mode, params, gamma, y0=y0, x0=x0))
            need = L.dp_ordered_workspace_bytes(n, h, w)
            io, oo = ORD_OFFS[aligned][i % len(ORD_OFFS[aligned])]
            assert ((io | oo) & 3 == 0) == aligned and (not aligned or (io & 7 and oo & 7))   # 4-byte aligned and no better

            def call(p, ws, wsb):
                assert ((p["in"] | p["out"]) & 3 == 0) == aligned
                return L.dp_ordered_u8(p["in"], p["out"], n, h, w, y0, x0, P._h, m, thr._h if m == be.MODE_MATRIX else None,
                                       float(params.get("scale", 1.0)), int(params.get("seed", 0)), ws, wsb, be._stream())

            if capfd is not None:
                capfd.readouterr()
            run_op(L, "dp_ordered_u8", {"in": (frames, io)}, {"out": (frames.nbytes, oo)}, need, call,
                   lambda o: _eq(o["out"], want, f"{what} {mode} {(n, h, w)} origin {(y0, x0)} aligned={aligned}"),
                   frame_bytes=h * w * 3, misaligned=(i == 0), seed=seed0 + i)
            if capfd is not None:
                seen = re.findall(r"dp_ordered_u8: pass 1 = (\w+) \(4-byte aligned frames: (\d)\)", capfd.readouterr().err)
                assert len(seen) == len(FILLS), seen                     # one launch per fill; the refused calls launch nothing
                for fam, al in seen:
                    assert (al == "1") == aligned, (what, mode, seen)
                    assert (fam == expect[mode]) if aligned else (fam in FALLBACK), (what, mode, (n, h, w), aligned, seen, expect)
                    reached.add(fam)
            i += 1
    return reached


def _ordered_family(orc, family):
    """-> palette, use_gamma, accel, the pass-1 family per mode that 4-byte aligned frames must reach."""
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer

    def same(f):
        return {m: f for m in MODES}

    if family == "brute16":        # no accelerator: the brute-force kernels whatever the address
        return orc.palr(16, 3), False, False, same("brute")
    if family == "lean256":        # the lean table, K = 256 integer; nearest-only mode stages it nearest-first (the fast kernel)
        return orc.palr(256, 21), False, True, {"none": "fast", "bayer": "lean", "IGN": "lean"}
    if family == "compact64":      # an image-derived palette crowds few cells: the compact kernel by the library's own choice
        return ColorReducer.reduce_colors(Image.fromarray(orc.imgl(120, 203, 5, "smooth"), "RGB"), 64), False, True, same("compact")
    if family == "compactfloat256":   # use_gamma: the one-byte-per-entry float table
        return orc.palr(256, 31), True, True, same("compact_float")
    if family == "lean300":        # K > 256 on the integer table
        return orc.palr(300, 2), False, True, same("lean")
    if family == "brutefloat300":  # K > 256 under use_gamma: no table, the float64 brute-force kernel
        return orc.palr(300, 2), True, True, same("brute")
    raise ValueError(family)


ORD_FAMILIES = ["brute16", "lean256", "compact64", "compactfloat256", "lean300", "brutefloat300"]


@pytest.mark.parametrize("family", ORD_FAMILIES)
def test_ordered_product_kernels(gpu, orc, family):
    """The library that ships, every family at 4-byte aligned and at odd addresses; pixel counts that are not a multiple of
    256 (the flag bitmap's tail), several tiles, more tiles than workgroups, tile origins.  The family each case reaches is
    the one test_ordered_kernel_families_traced asserts for the same case on the experiments build."""
    L, be = gpu
    pal, gamma, accel, _ = _ordered_family(orc, family)
    _ordered_cases(L, be, orc, pal, gamma, accel, ORD_SHAPES, family, 100, big=ORD_BIG)


@pytest.mark.parametrize("family", ORD_FAMILIES)
def test_ordered_kernel_families_traced(gpu, orc, switches, capfd, family):
    """The same cases on the experiments build with DP_ORDERED_TRACE=1 as its only switch: every 4-byte aligned case must
    reach the family's kernel, every odd-address case the fall-back kernels."""
    from dither_pie_amd import _lib, backend as be
    switches.setenv("DP_ORDERED_TRACE", "1")
    pal, gamma, accel, expect = _ordered_family(orc, family)
    reached = _ordered_cases(_lib.load(), be, orc, pal, gamma, accel, ORD_SHAPES, family, 100, expect=expect, capfd=capfd, big=ORD_BIG)
    assert set(expect.values()) <= reached and reached & FALLBACK


@pytest.mark.parametrize("pal_kind,env,expect", [
    ("img64", {"DP_FORCE_TABLE": "w8", "DP_FORCE_COMPACT": "1"}, "compact"),          # warped cells, compact kernel forced
    ("img64", {"DP_FORCE_TABLE": "u4"}, "compact"),                                     # plain cells, 4-entry blocks
    ("palr256", {"DP_FORCE_COMPACT": "1"}, "compact"),                                  # the compact kernel on an uncrowded palette
    ("palr256", {"DP_FORCE_TABLE": "u4"}, None),                                        # 4-entry blocks: fast (nearest) / lean
    ("gamma256", {"DP_NO_COMPACT_KERNEL": "1"}, "lean_float"),                          # use_gamma without the compact float kernel
    ("gamma64", {"DP_FORCE_TABLE": "w8", "DP_FORCE_COMPACT": "1"}, "compact_float"),    # compact float, image-derived, use_gamma
], ids=["img64-w8-compact", "img64-u4", "palr256-compact", "palr256-u4", "gamma256-leanfloat", "gamma64-compactfloat"])
def test_ordered_forced_tables(gpu, orc, switches, capfd, pal_kind, env, expect):
    """Forced cell tables (DP_FORCE_TABLE) and kernels (DP_FORCE_COMPACT, DP_NO_COMPACT_KERNEL), the family checked by trace."""
    from PIL import Image
    from dither_pie_amd import _lib, backend as be
    from dither_pie_amd.dithering_lib import ColorReducer
    for k, v in env.items():
        switches.setenv(k, v)
    switches.setenv("DP_ORDERED_TRACE", "1")
    img = ColorReducer.reduce_colors(Image.fromarray(orc.imgl(120, 203, 5, "smooth"), "RGB"), 64)
    pal, gamma = {"img64": (img, False), "palr256": (orc.palr(256, 21), False), "gamma256": (orc.palr(256, 31), True),
                  "gamma64": (img, True)}[pal_kind]
    exp = {m: expect for m in MODES} if expect else {"none": "fast", "bayer": "lean", "IGN": "lean"}
    reached = _ordered_cases(_lib.load(), be, orc, pal, gamma, True, SHAPES + [(2, 37, 53), (2, 61, 67)], f"{pal_kind} {env}", 200,
                             expect=exp, capfd=capfd)
    assert set(exp.values()) <= reached


# ================================================================================================ error diffusion
def _ed_case(L, be, orc, i, n, h, w, pal, variant, serp, gamma=False, what=""):
    P = be.Palette(*orc.prepare_palette(pal, gamma), accel=True)
    taps, div = orc.ed_kernel(variant)
    dx = np.array([t[0] for t in taps], np.int32)
    dy = np.array([t[1] for t in taps], np.int32)
    wq = np.array([t[2] / div for t in taps], np.float64).astype(np.float32)
    frames = _frames(orc, n, h, w, 300 + i)
    params = {"variant": variant, "serpentine": "true" if serp else "false"}
    want = _per_frame(frames, lambda f: orc.apply_dithering(f, pal, "error_diffusion", params, gamma))
    need = L.dp_error_diffusion_workspace_bytes(n, h, w)
    assert need == n * w * 96 + 512 + n * 256
    io, oo = OFFS[i % len(OFFS)]

    def call(p, ws, wsb):
        return L.dp_error_diffusion_u8(p["in"], p["out"], n, h, w, P._h, be._np_ptr(dx), be._np_ptr(dy), be._np_ptr(wq), len(taps),
                                       1 if serp else 0, ws, wsb, be._stream())

    run_op(L, "dp_error_diffusion_u8", {"in": (frames, io)}, {"out": (frames.nbytes, oo)}, need, call,
           lambda o: _eq(o["out"], want, f"error diffusion {what} {(n, h, w)} K={len(pal)} {variant} serp={serp}"),
           frame_bytes=h * w * 3, seed=300 + i)


def test_error_diffusion(gpu, orc):
    """One workgroup per frame, bands spread over workgroups (one 260-row frame), serpentine in LDS and the frame-parallel
    serpentine kernel with its error rows in the workspace (w = 5001); K <= 16, 17..256, > 256."""
    L, be = gpu
    pals = [orc.generate_uniform_palette(16), orc.palr(40, 9), orc.palr(300, 9)]
    i = 0
    for (n, h, w) in SHAPES + [(2, 70, 45)]:
        for pal, variant, serp in zip(pals, ("floyd_steinberg", "jjn", "atkinson"), (False, True, False)):
            _ed_case(L, be, orc, i, n, h, w, pal, variant, serp)
            i += 1
    for pal in pals:                                                 # >= 4 bands, w >= 64, few frames: the spread schedule
        _ed_case(L, be, orc, i, 1, 260, 67, pal, "floyd_steinberg", False, what="spread")
        i += 1
    _ed_case(L, be, orc, i, 2, 260, 67, pals[0], "stucki", False, gamma=True, what="spread, two frames")
    _ed_case(L, be, orc, i + 1, 1, 5, 4300, pals[0], "sierra", True, what="serpentine in LDS")
    _ed_case(L, be, orc, i + 2, 1, 3, 5001, pals[0], "sierra", True, what="serpentine rows in the workspace")
    _ed_case(L, be, orc, i + 3, 3, 3, 5001, pals[1], "floyd_steinberg", True, what="serpentine rows in the workspace")


def test_error_diffusion_persistent_grid(gpu, orc, switches):
    """More frames than workgroups (DP_ED_GRID): waves run on into the next frame's bands."""
    from dither_pie_amd import _lib, backend as be
    switches.setenv("DP_ED_ONE_WG", "1")
    switches.setenv("DP_ED_GRID", "2")
    L = _lib.load()
    _ed_case(L, be, orc, 40, 5, 333, 23, orc.generate_uniform_palette(16), "floyd_steinberg", False, what="persistent")
    _ed_case(L, be, orc, 41, 5, 290, 21, orc.palr(40, 9), "sierra_lite", False, what="persistent")


def test_numba_arithmetic(gpu, orc):
    """dp_error_diffusion_numba_u8 (both scans) and dp_hybrid_numba_u8: float64 error rings, the '3 doubles' of the size query."""
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(2, 70, 45), (1, 260, 67), (1, 3, 5001)]:
        for serp in (False, True):
            pal = orc.palr(16, 3) if i % 2 else orc.generate_uniform_palette(16)
            pal_f32, oc, lut = orc.prepare_palette(pal, i % 3 == 2)
            P = be.Palette(pal_f32, oc, lut)
            taps, div = orc.ed_kernel("jjn" if i % 2 else "floyd_steinberg")
            variant = "jjn" if i % 2 else "floyd_steinberg"
            dx = np.array([t[0] for t in taps], np.int32)
            dy = np.array([t[1] for t in taps], np.int32)
            wts = np.array([t[2] for t in taps], np.float32)
            frames = _frames(orc, n, h, w, 400 + i)
            need = L.dp_error_diffusion_workspace_bytes(n, h, w)
            io, oo = OFFS[i % len(OFFS)]
            want = _per_frame(frames, lambda f: orc.error_diffusion_numba_u8(f, pal_f32, oc, lut, variant, serp))

            def call(p, ws, wsb):
                return L.dp_error_diffusion_numba_u8(p["in"], p["out"], n, h, w, P._h, be._np_ptr(dx), be._np_ptr(dy), be._np_ptr(wts),
                                                     float(div), len(taps), 1 if serp else 0, ws, wsb, be._stream())

            run_op(L, "dp_error_diffusion_numba_u8", {"in": (frames, io)}, {"out": (frames.nbytes, oo)}, need, call,
                   lambda o: _eq(o["out"], want, f"numba arithmetic {(n, h, w)} serp={serp}"), frame_bytes=h * w * 3, seed=400 + i)
            if not serp:
                wanth = _per_frame(frames, lambda f: orc.hybrid_numba_u8(f, pal_f32, oc, lut, 1.4, 0.3))

                def callh(p, ws, wsb):
                    return L.dp_hybrid_numba_u8(p["in"], p["out"], n, h, w, P._h, 1.4, 0.3, ws, wsb, be._stream())

                run_op(L, "dp_hybrid_numba_u8", {"in": (frames, oo)}, {"out": (frames.nbytes, io)}, need, callh,
                       lambda o: _eq(o["out"], wanth, f"hybrid numba {(n, h, w)}"), frame_bytes=h * w * 3, seed=450 + i)
            i += 1


# ================================================================================================ variable diffusers, gate
VAR_MODES = [("perceptual", {}, 1, False), ("hybrid", {"lum_factor": 1.4, "col_factor": 0.3}, 2, False),
             ("adaptive_variance", {"var_threshold": 200.0, "window_radius": 2}, 3, False),
             ("ostromoukhov", {"serpentine": "false"}, 4, False), ("ostromoukhov", {"serpentine": "true"}, 4, True)]


def _var_case(L, be, orc, i, n, h, w, pal, gamma, mode, params, model, serp, what=""):
    pal_f32, oc, lut = orc.prepare_palette(pal, gamma)
    P = be.Palette(pal_f32, oc, lut, accel=True)
    frames = _frames(orc, n, h, w, 500 + i)
    want = _per_frame(frames, lambda f: orc.apply_dithering(f, pal, mode, params, gamma))
    need = L.dp_error_diffusion_workspace_bytes(n, h, w)
    io, oo = OFFS[i % len(OFFS)]
    inputs = {"in": (frames, io)}
    if model == 3:    # the gate map: read-only, at an odd address
        inputs["gate"] = (_per_frame(frames, lambda f: orc.variance_gate(lut[f] if lut is not None else f, params["var_threshold"],
                                                                         params["window_radius"])[0]), 5)
    if model == 4:    # the coefficient table: float32 at a 4-byte aligned address
        inputs["coef"] = (orc.ostromoukhov_coefficients(), 12)

    def call(p, ws, wsb):
        return L.dp_variable_diffusion_u8(p["in"], p["out"], n, h, w, P._h, model, float(params.get("lum_factor", 0.0)),
                                          float(params.get("col_factor", 0.0)), 1 if serp else 0, p.get("gate"), p.get("coef"), ws, wsb,
                                          be._stream())

    run_op(L, "dp_variable_diffusion_u8", inputs, {"out": (frames.nbytes, oo)}, need, call,
           lambda o: _eq(o["out"], want, f"{mode} {what} {(n, h, w)} K={len(pal)} gamma={gamma}"), frame_bytes=h * w * 3, seed=500 + i)


def test_variable_diffusion(gpu, orc):
    """The four diffusers and Ostromoukhov's serpentine scan; one workgroup per frame and bands spread over workgroups."""
    L, be = gpu
    i = 0
    for mode, params, model, serp in VAR_MODES:
        for (n, h, w) in SHAPES + [(2, 40, 50)]:
            _var_case(L, be, orc, i, n, h, w, orc.palr(16, 3) if i % 2 else orc.palr(300, 9), i % 3 == 1, mode, params, model, serp)
            i += 1
        _var_case(L, be, orc, i, 1, 290, 130, orc.palr(16, 8), False, mode, params, model, serp, what="spread")
        i += 1


def test_variable_diffusion_persistent_grid(gpu, orc, switches):
    from dither_pie_amd import _lib, backend as be
    switches.setenv("DP_ED_ONE_WG", "1")
    switches.setenv("DP_ED_GRID", "2")
    L = _lib.load()
    for i, (mode, params, model, serp) in enumerate(VAR_MODES[:4]):
        _var_case(L, be, orc, 60 + i, 5, 290, 23, orc.palr(16, 8), False, mode, params, model, serp, what="persistent")


def test_variance_gate(gpu, orc):
    """The fused path (radius <= 4) and the two-pass path with its float planes in the workspace (radius 5), use_gamma."""
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(2, 33, 47), (1, 77, 91)]:
        for radius, thr, gamma in ((1, 300.0, False), (5, 900.0, True), (3, 50.0, True), (6, 250.0, False)):
            pal_f32, oc, lut = orc.prepare_palette(orc.palr(16), gamma)
            P = be.Palette(pal_f32, oc, lut)
            frames = _frames(orc, n, h, w, 600 + i)
            want = _per_frame(frames, lambda f: orc.variance_gate(lut[f] if lut is not None else f, thr, radius)[0])
            need = L.dp_variance_gate_workspace_bytes(n, h, w)
            io, oo = OFFS[i % len(OFFS)]

            def call(p, ws, wsb):
                return L.dp_variance_gate_u8(p["in"], p["gate"], n, h, w, P._h, thr, radius, ws, wsb, be._stream())

            run_op(L, "dp_variance_gate_u8", {"in": (frames, io)}, {"gate": (n * h * w, oo)}, need, call,
                   lambda o: _eq(o["gate"], want, f"gate {(n, h, w)} radius {radius} gamma={gamma}"), frame_bytes=h * w * 3, seed=600 + i)
            i += 1


# ================================================================================================ riemersma
def test_riemersma(gpu, orc):
    """K <= 64, <= 256, > 256; h != w, so squares of the Hilbert curve off the image are skipped.  No workspace."""
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(2, 9, 20), (1, 33, 17)]:
        for K in (16, 100, 300):
            pal = orc.palr(K, K)
            gamma = i % 4 == 3
            P = be.Palette(*orc.prepare_palette(pal, gamma))
            frames = _frames(orc, n, h, w, 700 + i)
            want = _per_frame(frames, lambda f: riemersma_ref.apply(f, pal, gamma))
            io, oo = OFFS[i % len(OFFS)]
            run_op(L, "dp_riemersma_u8", {"in": (frames, io)}, {"out": (frames.nbytes, oo)}, 0,
                   lambda p, ws, wsb: L.dp_riemersma_u8(p["in"], p["out"], n, h, w, P._h, be._stream()),
                   lambda o: _eq(o["out"], want, f"riemersma {(n, h, w)} K={K}"), frame_bytes=h * w * 3, seed=700 + i)
            i += 1


# ================================================================================================ halftone
HT_PARAMS = [dict(dot_gain=1.0, shape="circle"), dict(dot_gain=2.0, shape="square", cell_size=3), dict(dot_gain=0.5, shape="diamond", angle=30.0),
             dict(dot_gain=2.5, shape="circle", sharpness=4.0)]
POW_PARAMS = dict(cell_size=8, angle=45.0, dot_gain=2.5, min_dot_size=0.0, max_dot_size=1.0, shape="circle", sharpness=4.0)
POW_H, POW_W, POW_PIXEL = 200, 256, 47940


def _pow_list(L, be, h, w, P):
    """The fix-up list of a pow-class geometry (sorted indices, np.power thresholds), through backend.halftone_fixups."""
    import torch
    idx, thr = be.halftone_fixups(torch.device("cuda", torch.cuda.current_device()), h, w, P)
    return idx.cpu().numpy().astype(np.int32), thr.cpu().numpy().astype(np.float32)


def _halftone_case(L, be, orc, i, n, h, w, pal, gamma, params):
    pal_f32, oc, lut = orc.prepare_palette(pal, gamma)
    P = be.Palette(pal_f32, oc, lut)
    full = dict(halftone_ref.DEFAULTS, **params)
    hp = be.halftone_params(P.pal_f32, **full)
    frames = _frames(orc, n, h, w, 800 + i)
    if h * w > 1:
        frames[-1] = orc.imgl(h, w, i)
    want = _per_frame(frames, lambda f: halftone_ref.apply(f, pal, gamma, **full))
    inputs = {"in": (frames, OFFS[i % len(OFFS)][0])}
    need = L.dp_halftone_workspace_bytes(n, h, w, C.byref(hp))
    assert need > 0
    if hp.exp_class == be.HT_EXP_POW:
        ids, thr = _pow_list(L, be, h, w, hp)
        if len(ids):
            inputs["fix_idx"], inputs["fix_thr"] = (ids, 4), (thr, 12)   # int32 / float32 lists at 4-byte aligned addresses

    def call(p, ws, wsb):
        if "fix_idx" in p:
            hp.fix_idx_dev, hp.fix_thr_dev, hp.n_fix = p["fix_idx"], p["fix_thr"], len(inputs["fix_idx"][0])
        return L.dp_halftone_u8(p["in"], p["out"], n, h, w, P._h, C.byref(hp), ws, wsb, be._stream())

    run_op(L, "dp_halftone_u8", inputs, {"out": (frames.nbytes, OFFS[i % len(OFFS)][1])}, need, call,
           lambda o: _eq(o["out"], want, f"halftone {(n, h, w)} K={len(pal)} gamma={gamma} {params}"), frame_bytes=h * w * 3, seed=800 + i)
    return "fix_idx" in inputs


def test_halftone(gpu, orc):
    """The four exponent classes, the three shapes, K <= the leaf size and above it (duplicated entries: exact ties, the
    tie kernel), and the pow class with its fix-up list in read-only regions."""
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(2, 64, 65), (3, 31, 47)]:
        for params in HT_PARAMS:
            K = (8, 64, 300)[i % 3]
            pal = orc.palr(K, 5 + i)
            if K == 64:
                pal = pal[:32] + pal[:32]
            _halftone_case(L, be, orc, i, n, h, w, pal, i % 4 == 1, params)
            i += 1
    assert _halftone_case(L, be, orc, i, 1, POW_H, POW_W, orc.palr(16, 2), False, POW_PARAMS), "this geometry has a fix-up list"
    assert _halftone_case(L, be, orc, i + 1, 2, POW_H, POW_W, orc.palr(300, 2), False, POW_PARAMS)


def test_halftone_pow_flags_respects_cap(gpu, orc):
    """dp_halftone_pow_flags with a cap below the count it reports writes at most cap entries and still reports the count."""
    L, be = gpu
    hp = be.halftone_params(np.zeros((2, 3), np.float32), **POW_PARAMS)
    res = {}

    def make(cap, key):
        def call(p, ws, wsb):
            return L.dp_halftone_pow_flags(POW_H, POW_W, C.byref(hp), p["idx"] if cap else None, cap, p["count"], be._stream())

        def verify(o):
            c = int(o["count"].view(np.uint64)[0])
            ids = o["idx"].view(np.int32)[:min(c, cap)]
            assert len(set(ids.tolist())) == len(ids) and ((ids >= 0) & (ids < POW_H * POW_W)).all()
            res[key] = (c, np.sort(ids))
        return call, verify

    call, verify = make(4096, "full")
    run_op(L, "dp_halftone_pow_flags", {}, {"idx": (4096 * 4, 4), "count": (8, 8)}, 0, call, verify,
           compare=lambda o: {"count": o["count"]}, frame_bytes=POW_H * POW_W * 4, seed=850)
    count, full = res["full"]
    assert 1 <= count <= 4096 and POW_PIXEL in full
    cap = count - 1
    call, verify = make(cap, "capped")
    run_op(L, "dp_halftone_pow_flags", {}, {"idx": (cap * 4, 4), "count": (8, 8)}, 0, call, verify,
           compare=lambda o: {"count": o["count"]}, frame_bytes=POW_H * POW_W * 4, seed=851)
    assert res["capped"][0] == count and set(res["capped"][1].tolist()) <= set(full.tolist())
    # the other classes list nothing and still write the count
    hp2 = be.halftone_params(np.zeros((2, 3), np.float32), **dict(POW_PARAMS, dot_gain=2.0))
    run_op(L, "dp_halftone_pow_flags", {}, {"idx": (16, 4), "count": (8, 8)}, 0,
           lambda p, ws, wsb: L.dp_halftone_pow_flags(POW_H, POW_W, C.byref(hp2), p["idx"], 4, p["count"], be._stream()),
           lambda o: _eq(o["count"], np.zeros(8, np.uint8), "count of a class that lists nothing"),
           compare=lambda o: {"count": o["count"]}, seed=852)


# ================================================================================================ wavelet
def test_wavelet(gpu, orc):
    """Filter lengths 2, 4, 6, 8; subband_quant 1, small, 65536 (the wide path); a flat channel; the uniform stream in a
    read-only region of exactly n_uniforms doubles at an 8- but not 16-byte aligned address."""
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(2, 31, 47), (1, 64, 65)]:
        for wavelet, Q in (("haar", 8), ("db2", 1), ("coif1", 65536), ("db4", 3)):
            K = (16, 300, 10)[i % 3]
            pal = orc.palr(K, 9 + i)
            gamma = i % 4 == 2
            P = be.Palette(*orc.prepare_palette(pal, gamma))
            frames = _frames(orc, n, h, w, 900 + i)
            if i % 2:
                frames[0, ..., i % 3] = 77                              # a flat channel: its subbands draw nothing
            wid = wr.WAVELETS.index(wavelet)
            nu = L.dp_wavelet_uniforms_needed(h, w, wid)
            u = np.random.RandomState(42).random_sample(nu)
            want = _per_frame(frames, lambda f: wr.apply(f, pal, gamma, WL_TAPS, wavelet=wavelet, subband_quant=Q, seed=42))
            wp = be.WaveletParams(wid, Q, None, nu)
            need = L.dp_wavelet_workspace_bytes(n, h, w, C.byref(wp))
            assert need > 0
            io, oo = OFFS[i % len(OFFS)]

            def call(p, ws, wsb):
                wp.uniforms_dev = p["uniforms"]
                return L.dp_wavelet_u8(p["in"], p["out"], n, h, w, P._h, C.byref(wp), ws, wsb, be._stream())

            run_op(L, "dp_wavelet_u8", {"in": (frames, io), "uniforms": (u, 8)}, {"out": (frames.nbytes, oo)}, need, call,
                   lambda o: _eq(o["out"], want, f"wavelet {wavelet} Q={Q} {(n, h, w)} K={K} gamma={gamma}"), frame_bytes=h * w * 3,
                   seed=900 + i)
            i += 1


# ================================================================================================ resize, IGN field
def test_resize_nearest(gpu, orc):
    from PIL import Image
    L, be = gpu
    i = 0
    for (n, h, w) in SHAPES + [(3, 31, 47)]:
        for (oh, ow) in ((1, 1), (h * 3 + 1, w * 2 + 1), (max(1, h // 2), max(1, w // 3)), (7, 5)):
            frames = _frames(orc, n, h, w, 1000 + i)
            want = _per_frame(frames, lambda f: np.array(Image.fromarray(f).resize((ow, oh), Image.NEAREST)).reshape(oh, ow, 3))
            io, oo = OFFS[i % len(OFFS)]
            run_op(L, "dp_resize_nearest_u8", {"in": (frames, io)}, {"out": (n * oh * ow * 3, oo)}, 0,
                   lambda p, ws, wsb: L.dp_resize_nearest_u8(p["in"], p["out"], n, h, w, oh, ow, be._stream()),
                   lambda o: _eq(o["out"], want, f"resize {(n, h, w)} -> {(oh, ow)}"), frame_bytes=max(h * w, oh * ow) * 3, seed=1000 + i)
            i += 1


def test_ign_thresholds(gpu, orc):
    """The float32 field at a 4-byte but not 16-byte aligned address."""
    L, be = gpu
    for i, (h, w, y0, x0, scale, seed) in enumerate([(1, 1, 0, 0, 1.0, 0), (7, 1, 3, 9, 2.5, 17), (5, 7, 0, 0, 0.1, 9999), (37, 53, 11, 2, 1.7, 23)]):
        want = np.ascontiguousarray(orc.ign_thresholds(h, w, scale, seed, y0, x0), np.float32)
        run_op(L, "dp_ign_thresholds", {}, {"out": (h * w * 4, (4, 12, 4, 12)[i])}, 0,
               lambda p, ws, wsb: L.dp_ign_thresholds(p["out"], h, w, y0, x0, scale, seed, be._stream()),
               lambda o: _eq(o["out"], want.reshape(-1).view(np.uint8), f"IGN field {(h, w)}"), frame_bytes=h * w * 4, seed=1100 + i)


# ================================================================================================ k-means, distinct colours
def _hist_table_numpy(px):
    r, g, b = (px[:, i].astype(np.int64) for i in range(3))
    idx = ((r >> 4) << 20) | ((g >> 4) << 16) | ((b >> 4) << 12) | ((r & 15) << 8) | ((g & 15) << 4) | (b & 15)
    return np.bincount(idx, minlength=1 << 24).astype(np.uint32)


def test_kmeans_step(gpu, orc):
    """Pixel pointer at odd offsets, n not a multiple of 4 / 64 / 256, sums / counts / squared norms each exact-size with
    guards, with and without the mean of sklearn's tie rule."""
    L, be = gpu
    for i, (n, K) in enumerate([(1, 1), (3, 2), (255, 5), (1001, 32), (4099, 300), (70001, 16)]):
        rs = np.random.RandomState(i)
        px = rs.randint(0, 256, (n, 3)).astype(np.uint8) if i % 2 else rs.randint(0, 6, (n, 3)).astype(np.uint8) * 40
        centers = np.ascontiguousarray(px[rs.randint(0, n, K)].astype(np.float64) + (0.25 if i % 2 else 0.0))
        mean = orc.data_mean(px) if i % 2 == 0 else None
        s_ref, n_ref, inertia = orc.kmeans_step(px, centers, mean)
        inputs = {"px": (px, OFFS[i % len(OFFS)][0]), "centers": (centers, 8)}
        if mean is not None:
            inputs["mean"] = (np.ascontiguousarray(mean, np.float64), 8)

        def verify(o):
            s, c, q = o["sums"].view(np.int64).reshape(K, 3), o["counts"].view(np.int64), o["sumsq"].view(np.int64)
            assert np.array_equal(s, s_ref) and np.array_equal(c, n_ref), (n, K)
            x64 = px.astype(np.int64)
            assert int(q.sum()) == int((x64 * x64).sum())
            got = float((q - 2 * (centers * s).sum(1) + c * (centers * centers).sum(1)).sum())
            assert abs(got - inertia) <= 1e-9 * max(inertia, 1.0)

        run_op(L, "dp_kmeans_step_u8", inputs, {"sums": (K * 24, 8), "counts": (K * 8, 8), "sumsq": (K * 8, 8)}, 0,
               lambda p, ws, wsb: L.dp_kmeans_step_u8(p["px"], n, p["centers"], p.get("mean"), K, p["sums"], p["counts"], p["sumsq"],
                                                      be._stream()), verify, frame_bytes=n * 3, seed=1200 + i)


def test_kmeans_plusplus(gpu, orc):
    from dither_pie_amd import kmeans
    L, be = gpu
    for i, (n, K) in enumerate([(1, 1), (3, 2), (257, 5), (1001, 16)]):
        sample = np.random.RandomState(20 + i).randint(0, 256, (n, 3)).astype(np.uint8)
        if i == 2:
            sample[::3] = sample[0]                                   # duplicates: zero distances
        n_trials = 2 + int(np.log(K))
        rs = np.random.RandomState(5 + i)
        first = kmeans.first_center_draw(n, rs)
        uniforms = np.stack([rs.uniform(size=n_trials) for _ in range(1, K)]) if K > 1 else np.zeros((1, 1))
        c_ref, ids_ref = kmeans.kmeans_plusplus(sample, K, np.random.RandomState(5 + i), return_indices=True)

        def verify(o):
            assert np.array_equal(o["ids"].view(np.int32), ids_ref.astype(np.int32)), (n, K)
            assert np.array_equal(o["centers"].view(np.float64).reshape(K, 3), c_ref)

        run_op(L, "dp_kmeans_plusplus_u8", {"sample": (sample, OFFS[i][0]), "uniforms": (np.ascontiguousarray(uniforms), 8)},
               {"ids": (K * 4, 4), "centers": (K * 24, 8)}, 0,
               lambda p, ws, wsb: L.dp_kmeans_plusplus_u8(p["sample"], n, K, first, p["uniforms"], n_trials if K > 1 else 1, p["ids"],
                                                          p["centers"], be._stream()), verify, frame_bytes=n * 3, seed=1300 + i)


def test_distinct_first(gpu, orc):
    """Exact-size out (3 n bytes) and count word, an exact-size 16- but not 32-aligned workspace; ws + 8 is refused."""
    L, be = gpu
    for i, n in enumerate([1, 3, 1001, 70001]):
        rs = np.random.RandomState(30 + i)
        px = rs.randint(0, 256, (40, 3)).astype(np.uint8)[rs.randint(0, 40, n)] if i % 2 == 0 else rs.randint(0, 256, (n, 3)).astype(np.uint8)
        packed = (px[:, 0].astype(np.int64) << 16) | (px[:, 1].astype(np.int64) << 8) | px[:, 2]
        first = np.sort(np.unique(packed, return_index=True)[1])
        want = px[first]
        need = L.dp_distinct_first_workspace_bytes(n)

        def verify(o):
            nd = int(o["n_distinct"].view(np.int64)[0])
            assert nd == len(want), (n, nd)
            _eq(o["out"][:3 * nd], want.reshape(-1), f"distinct colours of {n} pixels")

        def compare(o):
            return {"n_distinct": o["n_distinct"], "out": o["out"][:3 * len(want)]}

        run_op(L, "dp_distinct_first_u8", {"px": (px, OFFS[i][0])}, {"out": (3 * n, OFFS[i][1]), "n_distinct": (8, 8)}, need,
               lambda p, ws, wsb: L.dp_distinct_first_u8(p["px"], n, p["out"], p["n_distinct"], ws, wsb, be._stream()), verify,
               frame_bytes=n * 3, misaligned=True, compare=compare, seed=1400 + i)


def test_kmeans_histogram_and_fit(gpu, orc):
    """dp_kmeans_hist_build_u8 into an exact-size histogram that held 0xFF / noise / zeros (accumulate = 0 must clear it) with
    an exact-size workspace; then, at two sizes, the build on 0xFF compared with numpy, dp_kmeans_hist_step with its outputs
    pre-filled three ways, and a whole fit inside the arena, once with dp_kmeans_hist_iterate and once with
    dp_kmeans_hist_step + dp_kmeans_update, against the oracle's Lloyd iteration."""
    import torch
    L, be = gpu
    HB = L.dp_kmeans_hist_bytes()
    for i, n in enumerate([1, 1001, 70001]):
        rs = np.random.RandomState(40 + i)
        px = orc.imgl(1, n, i).reshape(-1, 3) if i == 1 else rs.randint(0, 256, (n, 3)).astype(np.uint8)
        table = _hist_table_numpy(px)
        per_cell = table.reshape(4096, 4096).sum(1).astype(np.uint32)
        occupied = np.nonzero(per_cell)[0]
        need = L.dp_kmeans_hist_workspace_bytes(n)

        def parts(o):
            info = o["hist"][1 << 26:].view(np.uint32)
            return {"table": o["hist"][:1 << 26], "cells": info[:4097].copy(), "list": np.sort(info[4097:4097 + len(occupied)] & 0xfff),
                    "overflow": info[8193:8194].copy()}

        def verify(o):
            q = parts(o)
            assert np.array_equal(q["table"].view(np.uint32), table), n
            assert np.array_equal(q["cells"][:4096], per_cell) and q["cells"][4096] == len(occupied)
            assert np.array_equal(q["list"], occupied) and q["overflow"][0] == 0

        run_op(L, "dp_kmeans_hist_build_u8", {"px": (px, OFFS[i][0])}, {"hist": (HB, 0)}, need,
               lambda p, ws, wsb: L.dp_kmeans_hist_build_u8(p["px"], n, p["hist"], 0, ws, wsb, be._stream()), verify,
               frame_bytes=1, misaligned=True, compare=parts, seed=1500 + i)
    for n, K in ((20011, 7), (1003, 32)):
        _histogram_pass_and_fit(L, be, orc, HB, n, K)
    torch.cuda.empty_cache()


def _histogram_pass_and_fit(L, be, orc, HB, n, K):
    """One arena for pixels, histogram, workspace and every small buffer of a fit."""
    px = orc.imgl(1, n, 3).reshape(-1, 3)
    px[::5] = np.random.RandomState(1).randint(0, 256, (len(px[::5]), 3))
    mean = orc.data_mean(px)
    init = np.ascontiguousarray(px[np.random.RandomState(2).choice(n, K, replace=False)].astype(np.float64))
    c_ref, inertia_ref, it_ref = orc.kmeans_lloyd(px, init)
    s_ref, n_ref, _ = orc.kmeans_step(px, init, mean)
    g = ar.MIN_GUARD
    small = [(K * 24, g), (24, g), (K * 40, g), (K * 32, g), (64, g), (4, g), (K * 24, g), (K * 8, g), (K * 8, g)]
    need = L.dp_kmeans_hist_workspace_bytes(n)
    A = ar.Arena(ar.capacity_for([(n * 3, g), (HB, g), (need, g)] + small), "cuda", 9)
    A.carve("px", n * 3, 3, g)
    A.put("px", px)
    A.carve("hist", HB, 0, g)
    A.carve("ws", need, 0, g)
    # the build with accumulate = 0 into a histogram and a workspace that hold 0xFF: compared with numpy directly
    A.fill("hist", "ones")
    A.fill("ws", "ones")
    assert L.dp_kmeans_hist_build_u8(A.ptr("px"), n, A.ptr("hist"), 0, A.ptr("ws"), need, be._stream()) == DP_OK
    _sync()
    built = A.get("hist").copy()
    table = _hist_table_numpy(px)
    per_cell = table.reshape(4096, 4096).sum(1).astype(np.uint32)
    occupied = np.nonzero(per_cell)[0]
    info = built[1 << 26:].view(np.uint32)
    assert np.array_equal(built[:1 << 26].view(np.uint32), table), (n, "0xFF left in the table")
    assert np.array_equal(info[:4096], per_cell) and info[4096] == len(occupied) and info[8193] == 0
    assert np.array_equal(np.sort(info[4097:4097 + len(occupied)] & 0xfff), occupied)
    A.check()
    A.unchanged("px")
    A.put("hist", built)                                                 # from here on the histogram is an input
    for name, nb, off in (("centers", K * 24, 8), ("mean", 24, 8), ("totals", K * 40, 8), ("prev", K * 32, 8), ("status", 64, 8),
                          ("ticket", 4, 4), ("sums", K * 24, 8), ("counts", K * 8, 8), ("sumsq", K * 8, 8)):
        A.carve(name, nb, off, g)
    A.put("mean", mean)
    A.put("centers", init)
    for i, fill in enumerate(FILLS):                                     # the pass overwrites its outputs whatever they held
        A.reseed(60 + i)
        for name in ("sums", "counts", "sumsq"):
            A.fill(name, fill)
        assert L.dp_kmeans_hist_step(A.ptr("hist"), A.ptr("centers"), A.ptr("mean"), K, A.ptr("sums"), A.ptr("counts"), A.ptr("sumsq"),
                                     be._stream()) == DP_OK
        _sync()
        assert np.array_equal(A.get("sums", np.int64).reshape(K, 3), s_ref) and np.array_equal(A.get("counts", np.int64), n_ref), (n, K, fill)
        assert int(A.get("sumsq", np.int64).sum()) == int((px.astype(np.int64) ** 2).sum()), (n, K, fill)
        A.check()
        for name in ("hist", "centers", "mean", "px"):
            A.unchanged(name)
    # (totals / prev / status / ticket start at zero: the header requires it of totals, status and ticket, and says nothing else of prev)
    for fused in (True, False):
        A.reseed(50 + fused)
        A.put("centers", init)
        for name in ("totals", "prev", "status", "ticket"):
            A.fill(name, "zeros")
        base = A.ptr("totals")
        for launched in range(it_ref + 40):
            if fused:
                rc = L.dp_kmeans_hist_iterate(A.ptr("hist"), A.ptr("centers"), A.ptr("mean"), K, base, A.ptr("prev"), A.ptr("status"),
                                              A.ptr("ticket"), 1e-4, 300, 1 if launched == 0 else 0, be._stream())
            else:
                rc = L.dp_kmeans_hist_step(A.ptr("hist"), A.ptr("centers"), A.ptr("mean"), K, base, base + 24 * K,
                                           (base + 32 * K) if launched == 0 else None, be._stream())
                assert rc == DP_OK
                rc = L.dp_kmeans_update(base, A.ptr("centers"), A.ptr("prev"), A.ptr("status"), K, 1e-4, 300, be._stream())
            assert rc == DP_OK, L.dp_last_error()
        _sync()
        st = A.get("status", np.float64)
        assert int(st[0]) in (1, 3) and int(st[1]) == it_ref, (fused, st.tolist(), it_ref)
        assert np.abs(A.get("centers", np.float64).reshape(K, 3) - c_ref).max() < 1e-9, fused
        assert abs(st[2] - inertia_ref) <= 1e-9 * inertia_ref
        A.check()
        for name in ("hist", "mean", "px"):
            A.unchanged(name)
    del A


# ================================================================================================ positive controls
def test_control_an_output_one_frame_short_is_caught(gpu, orc):
    """No broken library needed: `out` is declared one frame short and the full batch is asked for; the last frame lands in
    the guard (live memory, at least one frame long) and check() must name out / after / offset 0."""
    L, be = gpu
    n, h, w = 3, 5, 7
    frames = _frames(orc, n, h, w, 1)
    P = be.Palette(*orc.prepare_palette(orc.palr(16), False))
    g = ar.guard_bytes(h * w * 3)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), ((n - 1) * h * w * 3, g)]), "cuda", 4)
    A.carve("in", frames.nbytes, 1, g)
    A.put("in", frames)
    A.carve("out", (n - 1) * h * w * 3, 3, g)
    assert L.dp_riemersma_u8(A.ptr("in"), A.ptr("out"), n, h, w, P._h, be._stream()) == DP_OK
    _sync()
    with pytest.raises(ar.ArenaError) as e:
        A.check()
    assert (e.value.region, e.value.side, e.value.offset) == ("out", "after", 0) and 1 <= e.value.count <= h * w * 3
    _eq(A.get("out"), _per_frame(frames[:2], lambda f: riemersma_ref.apply(f, orc.palr(16), False)), "the frames that fit")


def test_control_a_written_read_only_region_is_caught(gpu, orc):
    """The read-only check on the device: a resize whose `out` is declared to be the read-only region changes it."""
    L, be = gpu
    frames = _frames(orc, 1, 5, 7, 2)
    g = ar.MIN_GUARD
    A = ar.Arena(ar.capacity_for([(105, g), (105, g)]), "cuda", 5)
    A.carve("in", 105, 1, g)
    A.put("in", frames)
    A.carve("table", 105, 3, g)
    A.fill("table", ar.noise(3))
    A.unchanged("table")
    assert L.dp_resize_nearest_u8(A.ptr("in"), A.ptr("table"), 1, 5, 7, 5, 7, be._stream()) == DP_OK
    _sync()
    A.check()
    with pytest.raises(ar.ArenaError) as e:
        A.unchanged("table")
    assert e.value.region == "table" and e.value.side == "inside"
    A.unchanged("in")


def test_control_an_op_that_reads_scratch_first_gives_fill_dependent_output(gpu, orc):
    """The stale-scratch check: a fake op (torch on arena views) that reads the workspace before writing it fails run_op's
    comparison across the three fills; the same op writing its scratch first passes."""
    L, _ = gpu
    x = np.arange(64, dtype=np.uint8)

    def op(read_first):
        def call(p, ws, wsb):
            A = p["arena"]
            src, dst, scr = (A.buf[a - A.base:a - A.base + 64] for a in (p["in"], p["out"], ws))
            if not read_first:
                scr.copy_(src)
            dst.copy_(scr + 1 if not read_first else src + scr)
            return DP_OK
        return call

    run_op(L, "fake", {"in": (x, 1)}, {"out": (64, 3)}, 64, op(False), lambda o: _eq(o["out"], x + 1, "fake op"), seed=7, refuse=False)
    with pytest.raises(AssertionError, match="depends on what the workspace held"):
        run_op(L, "fake", {"in": (x, 1)}, {"out": (64, 3)}, 64, op(True), lambda o: None, seed=8, refuse=False)
