"""GPU tier: every kernel instantiation and schedule the diffusion launchers can name, run for its VALUES and traced.

tests/diffusion_instances.py derives, from the conditions of launch_error_diffusion (csrc/ediff.hip), launch_variable_diffusion and
launch_variance_gate (csrc/vardiff.hip), one small case for every instantiation the launchers spell: the 42 + 2 wavefront instances
of plain error diffusion (three search kinds, seven tap counts, four or sixteen waves; the numba arithmetic), the row-serial kernels
of both families at the widest row that fits LDS and the lane = frame kernels at the next, the lane = frame kernels again at
w = 60000 with every arithmetic and model, the spread and persistent launches of each family, the fused gate per radius.  Each case
runs on the experiments library with DP_ED_TRACE=1 and asserts

  - the instance and the schedule the launcher's trace line names are the ones the row was derived for, and
  - the bytes equal the C oracle's, in index colours (out_colors[k] spells k), with no tolerance;

test_cases_cover_the_instances then asserts that the traced set is NAMED - UNREACHED and that every family took every schedule.

test_model3_gate_maps (the library that ships): adaptive variance with gate maps given directly -- closed, open, checkerboard, one
open pixel per corner, the last column -- whose open bytes are 1, 2, 128 and 255, at widths around the wavefront kernel's 16-byte
gate fetch and heights around its 64-row bands, one and three frames, one map per width carved at an odd address.

Measured on one MI355X: the module (174 tests) takes 60 s; the slowest cases are the lane = frame kernels with 300 colours, 2.5 to 4.3 s
(the numba arithmetic scans the palette in float64 at each of 180 000 sequential steps of (2, 3, 60000)); everything else is under 2 s, the
wavefront and row-serial cases under 0.3 s."""
import numpy as np
import pytest

import arena as ar
import cube_ref as cr
import diffusion_instances as di

pytestmark = pytest.mark.gpu

_REACHED = {}     # case id -> (instance, schedule) as traced
_ORACLE = {}      # (case id) -> what the oracle answered for the distinct frames


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


def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _taps(orc, name):
    return di.CUSTOM_TAPS[name] if name in di.CUSTOM_TAPS else orc.ed_kernel(name)


GATE_BYTES = (0, 0, 1, 2, 128, 255)      # closed twice as often as each open value; the oracle takes any non-zero byte as open


def _inputs(orc, case):
    """the distinct frames of the case (and their gate maps for model 3)"""
    _, h, w = case.shape
    kind, seed, distinct = case.content
    assert kind == "rnd"
    frames = [orc.rnd(h, w, 1000 * seed + i) for i in range(distinct)]
    gates = None
    if case.params.get("model") == 3 and "gate_pattern" in case.params:      # a map of _gate_patterns, its open bytes shifted per frame
        gates = [_gate_bytes(_gate_patterns(h, w)[case.params["gate_pattern"]], i) for i in range(distinct)]
    elif case.params.get("model") == 3:
        rs = np.random.RandomState(seed)
        gates = [np.array(GATE_BYTES, np.uint8)[rs.randint(0, len(GATE_BYTES), (h, w))] for _ in range(distinct)]
    return frames, gates


def _oracle(orc, case, pal_f32, oc, frames, gates):
    if case.id not in _ORACLE:
        p = case.params
        out = []
        for i, arr in enumerate(frames):
            if case.entry == "error_diffusion":
                taps, div = _taps(orc, p["taps"])
                out.append(orc.error_diffusion_u8(arr, pal_f32, oc, None, serpentine=p["serpentine"], taps=taps, div=div))
            elif case.entry == "error_diffusion_numba":
                taps, div = _taps(orc, p["taps"])
                out.append(orc.error_diffusion_numba_u8(arr, pal_f32, oc, None, serpentine=p["serpentine"], taps=taps, div=div))
            elif case.entry == "hybrid_numba":
                out.append(orc.hybrid_numba_u8(arr, pal_f32, oc, None, p["lum_factor"], p["col_factor"]))
            elif case.entry == "variable_diffusion":
                p0, p1 = (1.0, 0.2) if p["model"] == 2 else (0.0, 0.0)
                out.append(orc.var_diffusion_u8(arr, pal_f32, oc, None, p["model"], p0, p1, serpentine=p["serpentine"],
                                                gate=gates[i] if gates else None))
            else:
                out.append(orc.variance_gate(arr, p["var_threshold"], p["window_radius"])[0])
        _ORACLE[case.id] = out
    return _ORACLE[case.id]


def _launch(be, orc, case, P, frames, gates):
    """the case's one call on the device -> the output tensor"""
    import torch
    n = di.frames_of(case.shape, _cus())
    p = case.params
    x = torch.from_numpy(np.stack([frames[i % len(frames)] for i in range(n)])).cuda()
    if case.entry == "error_diffusion" or case.entry == "error_diffusion_numba":
        taps, div = _taps(orc, p["taps"])
        return be.error_diffusion(x, P, taps, div, p["serpentine"], arithmetic="numba" if case.entry.endswith("numba") else "python")
    if case.entry == "hybrid_numba":
        return be.hybrid_numba(x, P, p["lum_factor"], p["col_factor"])
    if case.entry == "variable_diffusion":
        p0, p1 = (1.0, 0.2) if p["model"] == 2 else (0.0, 0.0)
        g = torch.from_numpy(np.stack([gates[i % len(gates)] for i in range(n)])).cuda() if gates else None
        coef = torch.from_numpy(orc.ostromoukhov_coefficients()).cuda() if p["model"] == 4 else None
        return be.variable_diffusion(x, P, p["model"], p0, p1, serpentine=p["serpentine"], gate=g, coef=coef)
    return be.variance_gate(x, P, p["var_threshold"], p["window_radius"])


def _traced(capfd, case):
    import torch
    torch.cuda.synchronize()
    t = di.parse_trace(capfd.readouterr().err)
    assert len(t) == 1, f"{case.id}: one call, {len(t)} trace lines: {t}"
    return t[0]


def _palette(be, orc, name):
    pal_f32 = di.palette_f32(orc, name)
    oc = cr.index_colours(len(pal_f32))
    return pal_f32, oc, be.Palette(pal_f32, oc, None, accel=True)


def _setup(mp, case):
    for k, v in case.switches.items():
        mp.setenv(k, v)
    mp.setenv("DP_ED_TRACE", "1")
    from dither_pie_amd import backend
    return backend


@pytest.mark.parametrize("case", di.CASES, ids=lambda c: c.id)
def test_instance_values_and_trace(orc, switches, capfd, case):
    be = _setup(switches, case)
    pal_f32, oc, P = _palette(be, orc, case.pal)
    frames, gates = _inputs(orc, case)
    want = _oracle(orc, case, pal_f32, oc, frames, gates)
    capfd.readouterr()
    got = _launch(be, orc, case, P, frames, gates)
    t = _traced(capfd, case)
    _REACHED[case.id] = (t.instance, getattr(t, "schedule", None))
    got = got.cpu().numpy()
    # which kernel, which schedule
    assert t.instance == case.expect[0], f"{case.id}: traced {t}, derived {case.expect} from: {case.why}"
    if case.entry == "variance_gate":
        assert t.radius == case.params["window_radius"] and t.chunk == case.shape[0]
    else:
        assert t.schedule == case.expect[1], f"{case.id}: traced {t}, derived {case.expect} from: {case.why}"
        assert (t.K, t.n_inner) == (di.PALETTES[case.pal], di.N_INNER[case.pal]), t
        assert t.repair == (1 if t.schedule == "spread" else 0) and (t.G > 1) == (t.schedule == "spread")
        if t.schedule == "persistent":
            assert t.grid < got.shape[0]
        if t.instance[0] == "ed_rowserial":
            assert t.lds == di.ed_rowserial_lds(case.shape[2], t.K) and t.lds + 512 <= di.LDS_LIMIT
        if t.instance[0] == "os_rowserial":
            assert t.lds == di.os_rowserial_lds(case.shape[2], t.K) and t.lds + 512 <= di.LDS_LIMIT
    # the bytes
    for i in range(got.shape[0]):
        ref = want[i % len(want)]
        if not np.array_equal(got[i], ref):
            bad = np.argwhere((got[i] != ref).any(-1)) if ref.ndim == 3 else np.argwhere(got[i] != ref)
            pytest.fail(f"{case.id} ({t.instance}, {getattr(t, 'schedule', '')}): frame {i}: {len(bad)} pixels differ from the oracle, first (y, x) "
                        f"{bad[:5].tolist()}: device {got[i][tuple(bad[0])].tolist()}, oracle {ref[tuple(bad[0])].tolist()}")


def test_cases_cover_the_instances(orc, switches, capfd):
    """The traced instances of all rows are NAMED - UNREACHED, nothing of UNREACHED was reached, and the wavefront kernels of each
    family took each schedule.  A row that did not run in this session (a selection with -k) is launched here for its trace alone."""
    for case in di.CASES:
        if case.id in _REACHED:
            continue
        with pytest.MonkeyPatch.context() as mp:
            be = _setup(mp, case)
            _, _, P = _palette(be, orc, case.pal)
            frames, gates = _inputs(orc, case)
            capfd.readouterr()
            _launch(be, orc, case, P, frames, gates)
            t = _traced(capfd, case)
            _REACHED[case.id] = (t.instance, getattr(t, "schedule", None))
            del P
    reached = {}
    for cid, (inst, sched) in sorted(_REACHED.items()):
        reached.setdefault(inst, []).append(f"{cid} [{sched}]")
    with capfd.disabled():
        print(f"\ninstances the diffusion cases reached ({len(reached)} of {len(di.NAMED)} named, {len(di.UNREACHED)} unreachable):")
        for inst in sorted(reached, key=str):
            print(f"  {inst}: {len(reached[inst])} cases, e.g. {reached[inst][0]}")
    assert set(di.UNREACHED) <= di.NAMED and all(r.strip() for r in di.UNREACHED.values())
    assert not set(reached) - di.NAMED, sorted(set(reached) - di.NAMED, key=str)
    assert not set(reached) & set(di.UNREACHED), f"listed as unreachable but reached: {sorted(set(reached) & set(di.UNREACHED))}"
    assert set(reached) == di.NAMED - set(di.UNREACHED), f"no case reached {sorted(di.NAMED - set(di.UNREACHED) - set(reached), key=str)}"
    family = {"error_diffusion": "python", "error_diffusion_numba": "numba", "hybrid_numba": "numba", "variable_diffusion": "variable"}
    took = {(family[c.entry], _REACHED[c.id][1]) for c in di.CASES if _REACHED[c.id][0][0] in ("ed_wavefront", "var_wavefront")}
    assert took == {(f, s) for f in di.FAMILIES for s in di.SCHEDULES}, sorted(took)


# ==================================================================================================== model 3 gate maps
GATE_WIDTHS = (1, 3, 15, 16, 17, 63, 64, 65, 97)
GATE_HEIGHTS = (1, 64, 65, 130)
OPEN_BYTES = np.array([1, 2, 128, 255], np.uint8)


def _gate_patterns(h, w):
    """name -> bool [h, w]"""
    y, x = np.mgrid[0:h, 0:w]
    pats = {"closed": np.zeros((h, w), bool), "open": np.ones((h, w), bool), "checkerboard": (x + y) % 2 == 0, "last-column": x == w - 1}
    for name, (cy, cx) in (("corner-00", (0, 0)), ("corner-0w", (0, w - 1)), ("corner-h0", (h - 1, 0)), ("corner-hw", (h - 1, w - 1))):
        pats[name] = (y == cy) & (x == cx)
    return pats


def _gate_bytes(mask, k):
    """open pixels take 1, 2, 128, 255 in turn (by position, shifted by k); closed ones are 0"""
    h, w = mask.shape
    y, x = np.mgrid[0:h, 0:w]
    return np.where(mask, OPEN_BYTES[(x + 3 * y + k) % 4], 0).astype(np.uint8)


@pytest.mark.parametrize("w", GATE_WIDTHS)
def test_model3_gate_maps(be, orc, w):
    import torch
    pal_f32 = di.palette_f32(orc, "palr40")
    oc = cr.index_colours(len(pal_f32))
    P = be.Palette(pal_f32, oc, None, accel=True)
    odd_done = False
    for h in GATE_HEIGHTS:
        imgs = [orc.rnd(h, w, 7000 + 10 * w + i) for i in range(3)]
        for n in (1, 3):
            for k, (name, mask) in enumerate(_gate_patterns(h, w).items()):
                # (three frames: the pattern on every frame, its open bytes shifted per frame)
                gates = np.stack([_gate_bytes(mask, k + i) for i in range(n)])
                want = np.stack([orc.var_diffusion_u8(imgs[i], pal_f32, oc, None, 3, gate=gates[i]) for i in range(n)])
                x = torch.from_numpy(np.stack(imgs[:n])).cuda()
                A = None
                if not odd_done and h == 65 and n == 3 and name == "checkerboard":    # one map per width at an odd address
                    A = ar.Arena(ar.capacity_for([(gates.size, ar.MIN_GUARD)]), device="cuda", seed=w)
                    g = A.carve("gate", gates.size, offset_mod16=1, guard=ar.MIN_GUARD).view(n, h, w)
                    A.put("gate", gates)
                    assert g.data_ptr() % 2 == 1
                    odd_done = True
                else:
                    g = torch.from_numpy(gates).cuda()
                got = be.variable_diffusion(x, P, 3, gate=g).cpu().numpy()
                if A is not None:
                    A.check()
                    A.unchanged("gate")
                if not np.array_equal(got, want):
                    bad = np.argwhere((got != want).any(-1))
                    pytest.fail(f"model 3, gate '{name}' ({'odd address' if A is not None else 'aligned'}), {n} x {h} x {w}: {len(bad)} pixels differ from "
                                f"the oracle, first (frame, y, x) {bad[:5].tolist()}")
    assert odd_done
