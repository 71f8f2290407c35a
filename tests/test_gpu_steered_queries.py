"""GPU tier: the nearest-colour search of the diffusion kernels at steered FRACTIONAL and OUT-OF-CUBE query points.

tests/test_gpu_colour_cube.py part (d) proves the candidate structures at every integer point of the cube.  Here the query of a
chosen pixel is put on a chosen float32 point (tests/steer_ref.py: one known push per receiver) -- between the last integer of a
16^3 cell or a 2-wide leaf and its face, clamped onto the faces, edges and corners of the cube, on near ties from float32's epsilon
up to 1e-4 of the squared distance, exact ties at fractional points, and beyond the cube in all 26 directions -- and the device's
bytes must equal the CPU oracle's, in index colours (out_colors[k] spells k), with no tolerance.  tests/test_steer_cpu.py shows,
from the points the oracle itself reports, that the frames ask what they are meant to ask.

  error diffusion, pair layout (N, H, 2), all sixteen weights 2^-1 .. 2^-16 per case:
      H = 256                      the four-wave instance, tables in LDS
      H = 1024, N <= CUs           the sixteen-wave instance, one workgroup per frame
      H = 320,  N  > CUs           the persistent grid, tables read from L2
      serpentine                   ed_rowserial_kernel
      arithmetic="numba"           the 4- and 8-wave numba instances; serpentine: ed_serial_kernel<., true>
      experiments library          the three raster python-arithmetic shapes again with each entry of test_gpu_colour_cube.ED_FORCED, on
                                   the four palettes that have an H4 table (as the cube test does); the numba arithmetic scans the
                                   whole palette, and serpentine is not repeated under the switches here, as it is not there
  (Serpentine and dup256 launch the full row sets too: about 20 000 rows a weight, under a second a case on one MI355X.)
  Ostromoukhov, pair layout, coefficient rows {w, 0, 0}: var_wavefront_kernel<., 4>; serpentine: os_rowserial_kernel
  adaptive variance, tile layout: one frame about 640 x 825 (the spread launch, its 64-row bands ordered inside-only / one outside
      pixel / targets outside for the __ballot branches), the same under DP_ED_ONE_WG and under DP_ED_TEST_GIVEUP (the repair
      launch), and more frames than CUs with five bands (the persistent grid)
  perceptual and hybrid: pair1 frames (N, 1, 2) -- one row, so one wave a frame and never the persistent grid -- and saturated
      frames hundreds to thousands of units beyond the cube (also adaptive variance with every gate on) in a few-frames shape
      and a persistent one
  palettes of <= 16 colours (nearest_ext, the coarse and expanded lists), 17 .. 256 (nearest_ext16, H4) and 257 .. 1024 (wide lists)
  (the per-lane searches named here are written once, in csrc/ed_nearest.hip.h: nearest_color, nearest_color_cells, nearest_ext,
  nearest_ext16, nearest_h4; so is wave_nearest, the per-wave scan of os_rowserial_kernel and riemersma_kernel -- ed_rowserial_kernel
  has its own copy of that scan in ediff.hip)

Left to the tests they have: the python-arithmetic ed_serial_kernel (test_serpentine_wide_rows_use_the_frame_parallel_kernel)
and var_serial_kernel, which is reached only by Ostromoukhov's serpentine scan on rows too wide for LDS (about 5000 pixels) or
at w >= 60000; neither layout here reaches them (test_ostromoukhov_serpentine_wide_rows in tests/test_gpu_kernels.py does, with
an exact tie at its first pixel).

A mismatch is a bug of the library at that point: the failure names the query point, its cell, the kind of target and the rung,
and the device's and the oracle's palette indices."""
import numpy as np
import pytest

import cube_ref as cr
import steer_ref as sr
from test_gpu_colour_cube import ED_FORCED

pytestmark = pytest.mark.gpu

CASES = [(n, g) for n in sr.PALETTES for g in cr.GAMMAS]
_ORACLE = {}      # (palette, gamma, what ...) -> the oracle's answer, computed once and shared by the shapes


@pytest.fixture
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    yield backend
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _ORACLE.clear()
    sr.release()


def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _palette(be, S):
    return be.Palette(S.pal, S.out_colors, S.lut, accel=True)


def _fail(S, what, got, want, q, describe):
    """got / want: [n, 3] output bytes of the pixels in question, q their predicted queries (or None)"""
    bad = np.flatnonzero((got != want).any(1))
    lines = []
    for i in bad[:8]:
        where = describe(i) if describe else ""
        point = S.describe(q[i]) if q is not None else ""
        lines.append(f"{point} {where}: device {cr.decode(got[i])}, oracle {cr.decode(want[i])}")
    pytest.fail(f"{what}: {len(bad)} of {len(got)} pixels differ from the oracle; " + "; ".join(lines))


# ==================================================================================================== pair layout
def _pair_oracle(orc, S, k, serp, arith):
    key = (S.name, S.gamma, "pair", k, serp, arith)
    if key not in _ORACLE:
        frame, rx, q, sel = S.pair_frame(k, serp)
        w = sr.PAIR_WEIGHTS[k]
        if arith == "python":
            out = orc.error_diffusion_u8(frame, S.pal, S.out_colors, S.lut, serpentine=serp, taps=[(1, 0, w)], div=1.0)
        elif arith == "numba":
            out = orc.error_diffusion_numba_u8(frame, S.pal, S.out_colors, S.lut, serpentine=serp, taps=[(1, 0, w)], div=1.0)
        else:
            coef = np.zeros((256, 3), np.float32)
            coef[:, 0] = w
            out = orc.var_diffusion_u8(frame, S.pal, S.out_colors, S.lut, 4, serpentine=serp, coef=coef)
        _ORACLE[key] = (frame, q, sel, out)
    return _ORACLE[key]


def _pair_shape(shape, R, cus):
    """(N, H) of a launch over R rows (rows are dealt cyclically; H is even, so a row keeps its parity)"""
    if shape == "four-wave":
        return -(-R // 256), 256
    if shape == "sixteen-wave":
        return max(1, min(cus, -(-R // 1024))), 1024
    if shape == "persistent":
        return cus + 8, 320
    if shape == "eight-wave":
        return max(1, -(-R // 512)), 512
    if shape == "rows64":
        return -(-R // 64), 64
    if shape == "rows32":
        return -(-R // 32), 32
    raise ValueError(shape)


def _pair_case(be, orc, name, gamma, shape, serp, arith, what=""):
    import torch
    S = sr.steer(orc, name, gamma)
    P = _palette(be, S)
    cus = _cus()
    for k, w in enumerate(sr.PAIR_WEIGHTS):
        frame, q, sel, out = _pair_oracle(orc, S, k, serp, arith)
        R = len(frame)
        N, H = _pair_shape(shape, R, cus)
        assert N * H >= R, f"{shape}: {N} x {H} rows do not hold the {R} rows whose coverage the CPU tier proves"
        rows = np.arange(N * H) % R
        frames = torch.from_numpy(frame[rows].reshape(N, H, 2, 3)).cuda()
        if arith == "ostromoukhov":
            coef = torch.zeros((256, 3), dtype=torch.float32, device="cuda")
            coef[:, 0] = w
            got = be.variable_diffusion(frames, P, 4, serpentine=serp, coef=coef)
        else:
            got = be.error_diffusion(frames, P, [(1, 0, w)], 1.0, serp, arithmetic=arith)
        got = got.cpu().numpy().reshape(-1, 3)
        want = out[rows].reshape(-1, 3)
        if not np.array_equal(got, want):
            r = S.rows[("pair", k)]

            def describe(i):
                row = sel[rows[i // 2]]
                extra = f" rung {sr.RUNG_NAMES[r['rung'][row]]}" if r["kind"][row] == sr.K_LADDER else ""
                return f"[{sr.KINDS[r['kind'][row]]}{extra}; frame {i // 2 // H} row {i // 2 % H} x {i % 2}]"
            _fail(S, f"{what or 'product library'}: {arith} pair layout {N} x {H} x 2, weight 2^-{k + 1}, serpentine={serp}: {name} gamma={gamma}",
                  got, want, q[rows].reshape(-1, 3), describe)


ED_SHAPES = [("four-wave", False, "python"), ("sixteen-wave", False, "python"), ("persistent", False, "python"), ("rows64", True, "python"),
             ("four-wave", False, "numba"), ("eight-wave", False, "numba"), ("rows32", True, "numba")]


@pytest.mark.parametrize("shape,serp,arith", ED_SHAPES, ids=[f"{s}-{'serp' if p else 'raster'}-{a}" for s, p, a in ED_SHAPES])
@pytest.mark.parametrize("name,gamma", CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in CASES])
def test_error_diffusion_pair_layout(be, orc, name, gamma, shape, serp, arith):
    _pair_case(be, orc, name, gamma, shape, serp, arith)


@pytest.mark.parametrize("serp", (False, True), ids=["raster", "serp"])
@pytest.mark.parametrize("name,gamma", CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in CASES])
def test_ostromoukhov_pair_layout(be, orc, name, gamma, serp):
    _pair_case(be, orc, name, gamma, "rows64" if serp else "four-wave", serp, "ostromoukhov")


FORCED_CASES = [(n, g, env, what, shape)
                for n in ("palr256", "clustered200", "mc64", "dup256")      # 17 .. 256 colours: the palettes with an H4 table
                for g in cr.GAMMAS for env, what in ED_FORCED for shape in ("four-wave", "sixteen-wave", "persistent")
                # (the pair layout is two pixels wide and never takes the spread launch, whose repair DP_ED_TEST_GIVEUP forces: one
                # shape shows that the switch changes nothing here; the tile layout below reaches the repair launch)
                if "DP_ED_TEST_GIVEUP" not in env or shape == "four-wave"]


@pytest.mark.parametrize("name,gamma,env,what,shape", FORCED_CASES,
                         ids=["-".join([n, "gamma" if g else "int", "+".join(k[6:] for k in env), sh]) for n, g, env, _, sh in FORCED_CASES])
def test_error_diffusion_pair_layout_forced_structures(orc, switches, name, gamma, env, what, shape):
    for k, v in env.items():
        switches.setenv(k, v)
    from dither_pie_amd import backend
    _pair_case(backend, orc, name, gamma, shape, False, "python", what=f"{env}: {what}")


# ==================================================================================================== tile layout
def _tile_oracle(orc, S, shape, banded):
    key = (S.name, S.gamma, "tile", shape, banded)
    if key not in _ORACLE:
        frame, gate, q, tmap = S.tile_frames(*shape, banded=banded)
        out = np.stack([orc.var_diffusion_u8(frame[i], S.pal, S.out_colors, S.lut, 3, gate=gate[i]) for i in range(shape[0])])
        _ORACLE[key] = (frame, gate, q, tmap, out)
    return _ORACLE[key]


def _tile_case(be, orc, name, gamma, shape, banded, what):
    import torch
    S = sr.steer(orc, name, gamma)
    frame, gate, q, tmap, out = _tile_oracle(orc, S, shape, banded)
    got = be.variable_diffusion(torch.from_numpy(frame).cuda(), _palette(be, S), 3, gate=torch.from_numpy(gate).cuda()).cpu().numpy()
    if not np.array_equal(got, out):
        t = S.tiles()
        flat = tmap.reshape(-1)

        def describe(i):
            n, y, x = np.unravel_index(i, tmap.shape)
            if flat[i] < 0:
                return f"[frame {n} y {y} x {x}]"
            extra = f" rung {sr.RUNG_NAMES[t['rung'][flat[i]]]}" if t["kind"][flat[i]] == sr.K_LADDER else ""
            return f"[{sr.KINDS[t['kind'][flat[i]]]}{extra}; frame {n} y {y} x {x}, {sr.beyond(q.reshape(-1, 3)[i]):.1f} beyond the cube]"
        _fail(S, f"{what}: adaptive variance, tile layout {shape}: {name} gamma={gamma}", got.reshape(-1, 3), out.reshape(-1, 3), q.reshape(-1, 3), describe)


@pytest.mark.parametrize("name,gamma", CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in CASES])
def test_adaptive_variance_tile_layout_spread(be, orc, name, gamma):
    _tile_case(be, orc, name, gamma, sr.steer(orc, name, gamma).tile_spread_shape(), True, "the spread launch")


@pytest.mark.parametrize("name,gamma", CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in CASES])
def test_adaptive_variance_tile_layout_persistent(be, orc, name, gamma):
    _tile_case(be, orc, name, gamma, (_cus() + 8, 320, 12), False, "the persistent grid")


@pytest.mark.parametrize("env", ({"DP_ED_ONE_WG": "1"}, {"DP_ED_TEST_GIVEUP": "1"}), ids=["ONE_WG", "TEST_GIVEUP"])
@pytest.mark.parametrize("name,gamma", CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in CASES])
def test_adaptive_variance_tile_layout_forced(orc, switches, name, gamma, env):
    for k, v in env.items():
        switches.setenv(k, v)
    from dither_pie_amd import backend
    _tile_case(backend, orc, name, gamma, sr.steer(orc, name, gamma).tile_spread_shape(), True, f"{env}")


# ==================================================================================================== pair1 and saturate
PAIR1_CASES = sr.PAIR1_CASES      # (the CPU tier asserts the ladder floors of these very frames)
MODEL_ARGS = {1: {}, 2: dict(p0=1.0, p1=0.2)}


@pytest.mark.parametrize("model", (1, 2), ids=["perceptual", "hybrid"])
@pytest.mark.parametrize("name,gamma", PAIR1_CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in PAIR1_CASES])
def test_perceptual_and_hybrid_pair1_layout(be, orc, name, gamma, model):
    import torch
    S = sr.steer(orc, name, gamma)
    frames, q = S.pair1_frames(model, sr.PAIR1_FRAMES)
    want = np.stack([orc.var_diffusion_u8(f, S.pal, S.out_colors, S.lut, model, **MODEL_ARGS[model]) for f in frames])
    got = be.variable_diffusion(torch.from_numpy(frames).cuda(), _palette(be, S), model, **MODEL_ARGS[model]).cpu().numpy()
    if not np.array_equal(got, want):
        _fail(S, f"model {model}, pair1 layout: {name} gamma={gamma}", got.reshape(-1, 3), want.reshape(-1, 3), q.reshape(-1, 3),
              lambda i: f"[frame {i // 2} x {i % 2}, {sr.beyond(q.reshape(-1, 3)[i]):.1f} beyond the cube]")


SATURATE = [("mc256", False, ("white", "red", "green", "blue", "yellow", "ramp")), ("mc256", True, ("white", "blue", "ramp")),
            ("bright", False, ("black", "ramp")), ("palr16", False, ("white", "black", "ramp")), ("palr300", False, ("white", "black"))]


@pytest.mark.parametrize("shape", ("few", "persistent"))
@pytest.mark.parametrize("model", (1, 2, 3), ids=["perceptual", "hybrid", "adaptive"])
@pytest.mark.parametrize("pal_name,gamma,kinds", SATURATE, ids=[f"{p}-{'gamma' if g else 'int'}" for p, g, _ in SATURATE])
def test_saturated_frames(be, orc, pal_name, gamma, kinds, model, shape):
    """whole frames far from the palette's hull: the queries run hundreds to thousands of units beyond the cube (measured from the
    oracle's report in tests/test_steer_cpu.py), where the outermost extended cells stand for unbounded half-spaces"""
    import torch
    pal = sr.bright_palette(orc) if pal_name == "bright" else cr.palette(orc, pal_name)
    pal_f32, _, lut_in = orc.prepare_palette(pal, gamma)
    oc = cr.index_colours(len(pal_f32))
    n, h, w = (len(kinds), 256, 96) if shape == "few" else (_cus() + 8, 320, 8)
    base = sr.saturate_frames(h, w)
    gate = np.ones((h, w), np.uint8) if model == 3 else None
    kw = dict(MODEL_ARGS.get(model, {}))
    answers = {k: orc.var_diffusion_u8(base[k], pal_f32, oc, lut_in, model, gate=gate, **kw) for k in kinds}
    frames = np.stack([base[kinds[i % len(kinds)]] for i in range(n)])
    want = np.stack([answers[kinds[i % len(kinds)]] for i in range(n)])
    P = be.Palette(pal_f32, oc, lut_in, accel=True)
    gates = torch.ones((n, h, w), dtype=torch.uint8, device="cuda") if model == 3 else None
    got = be.variable_diffusion(torch.from_numpy(frames).cuda(), P, model, gate=gates, **kw).cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        f, y, x = bad[0]
        pytest.fail(f"model {model}, saturated frames {(n, h, w)} on {pal_name} gamma={gamma}: {len(bad)} pixels differ from the oracle; first: frame "
                    f"{f} ({kinds[f % len(kinds)]}) y {y} x {x}: device {cr.decode(got[f, y, x])}, oracle {cr.decode(want[f, y, x])}")
