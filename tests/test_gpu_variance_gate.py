"""GPU tier: dp_variance_gate_u8 against orc.variance_gate, every window radius path and the variance itself pinned to the bit.

The gate is `local variance >= threshold` with scipy's uniform_filter arithmetic (float64 running sums, float32 between the axes).
The fused kernel (radius <= 4, one instance per radius) replaces scipy's float64 division by a multiplication with a guarded
fallback (mean_f32, csrc/vardiff.hip); larger windows take two passes through a float32 workspace.  Here:

  test_gate_values        radii 0 1 2 3 4 5 6 8 33 64 (windows up to 129 wide, larger than every frame here) x shapes from one pixel
                          to a tile of 16 x 64 exactly, one pixel over in both axes, and three tiles a side x with / without lut_in;
                          three frames a call -- noise, orc.grad and a posterised frame whose flat patches have variance exactly 0 --
                          and one frame alone.  Thresholds are values the oracle's map takes and their float32 successors, so `>=`
                          against `>` shows.
  test_two_pass_switch    radii 0 .. 4 on the experiments library with DP_GATE_TWO_PASS: the trace says two_pass, the bytes are the
                          fused run's and the oracle's
  test_variance_is_pinned (17, 65) and (33, 47), every radius: one call per threshold, the thresholds being EVERY distinct value of the
                          oracle's float32 variance map and that value's successor.  A device variance below the oracle's at pixel p
                          fails at thr = var[p], one above it at the successor, so every pixel's variance is pinned to the bit.  The
                          maps are compared on the device, one copy back per case.
  test_threshold_edges    0.0, -0.0, -1.0, the smallest subnormal, inf and nan at radius 0 (variance exactly 0) and 2
  test_odd_input_address  frames carved at an odd address (the kernel reads a pixel as one unaligned dword)

Measured on one MI355X: the module (38 tests) takes 7 s; the slowest case is test_variance_is_pinned at radius 64 on (33, 47), 0.46 s for its
9 284 calls' worth of thresholds (4 642 distinct variances and their successors)."""
import numpy as np
import pytest

import arena as ar
import diffusion_instances as di

pytestmark = pytest.mark.gpu

RADII = (0, 1, 2, 3, 4, 5, 6, 8, 33, 64)
SHAPES = ((1, 1), (1, 7), (5, 1), (3, 200), (16, 64), (17, 65), (33, 47), (48, 80))
PINNED_SHAPES = ((17, 65), (33, 47))      # (17, 65): the smallest shape with two tiles on each axis
_REF = {}      # (shape, lut, radius) -> (frames, source the oracle saw, var maps)


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
    _REF.clear()


def posterised(h, w, seed):
    """flat patches of 5 x 9 pixels in colours of a few levels: a window that stays inside a patch has variance exactly 0"""
    rs = np.random.RandomState(seed)
    levels = rs.randint(0, 4, ((h + 4) // 5, (w + 8) // 9, 3)) * 85
    return np.ascontiguousarray(np.repeat(np.repeat(levels, 5, 0), 9, 1)[:h, :w].astype(np.uint8))


def _frames(orc, shape):
    h, w = shape
    return np.stack([orc.rnd(h, w, 31 * h + w), orc.grad(h, w), posterised(h, w, h + w)])


def _reference(orc, shape, lut, radius):
    """(frames uint8 [3, h, w, 3], the oracle's float32 variance maps [3, h, w]), computed once per (shape, lut, radius)"""
    key = (shape, lut, radius)
    if key not in _REF:
        frames = _frames(orc, shape)
        src = orc.gamma_luts()[0][frames] if lut else frames
        var = np.stack([orc.variance_gate(s, 0.0, radius)[1] for s in src])
        assert var.dtype == np.float32 and (var >= 0).all()
        _REF[key] = (frames, var)
    return _REF[key]


def _palette(be, orc, lut):
    pal_f32, out_colors, _ = orc.prepare_palette(orc.palr(16), False)
    return be.Palette(pal_f32, out_colors, orc.gamma_luts()[0] if lut else None)


def _some_thresholds(var):
    """per frame a value its map takes (the middle one of the distinct values) and that value's successor"""
    out = []
    for v in var:
        d = np.unique(v)
        out += [d[len(d) // 2], np.nextafter(d[len(d) // 2], np.float32(np.inf))]
    return out


def _check(got, var, thr, what):
    want = (var >= np.float32(thr)).astype(np.uint8)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        f, y, x = bad[0]
        pytest.fail(f"{what}, threshold {float(thr)!r}: {len(bad)} gate bytes differ from the oracle, first (frame, y, x) {bad[0].tolist()}: "
                    f"device {got[f, y, x]}, oracle variance {float(var[f, y, x])!r}")


@pytest.mark.parametrize("radius", RADII)
def test_gate_values(be, orc, radius):
    import torch
    for lut in (False, True):
        P = _palette(be, orc, lut)
        for shape in SHAPES:
            frames, var = _reference(orc, shape, lut, radius)
            x = torch.from_numpy(frames).cuda()
            for thr in _some_thresholds(var) + [300.0]:
                got = be.variance_gate(x, P, float(thr), radius)
                assert got.shape == (3,) + shape and got.dtype == torch.uint8
                _check(got.cpu().numpy(), var, thr, f"radius {radius}, 3 x {shape}, lut_in={lut}")
            thr = _some_thresholds(var[:1])[0]
            _check(be.variance_gate(x[:1], P, float(thr), radius).cpu().numpy(), var[:1], thr, f"radius {radius}, 1 x {shape}, lut_in={lut}")
    if radius == 0:
        assert not var.any()      # one pixel a window: gray^2 - gray * gray


@pytest.mark.parametrize("radius", (0, 1, 2, 3, 4))
def test_two_pass_switch(orc, switches, capfd, radius):
    import torch
    switches.setenv("DP_ED_TRACE", "1")
    from dither_pie_amd import backend as be
    for lut in (False, True):
        P = _palette(be, orc, lut)
        for shape in SHAPES:
            frames, var = _reference(orc, shape, lut, radius)
            x = torch.from_numpy(frames).cuda()
            for thr in _some_thresholds(var):
                switches.delenv("DP_GATE_TWO_PASS", raising=False)
                capfd.readouterr()
                fused = be.variance_gate(x, P, float(thr), radius)
                torch.cuda.synchronize()
                t = di.parse_trace(capfd.readouterr().err)
                assert [v.instance for v in t] == [("fused", radius)] and t[0].radius == radius and t[0].chunk == 3, t
                switches.setenv("DP_GATE_TWO_PASS", "1")
                two = be.variance_gate(x, P, float(thr), radius)
                torch.cuda.synchronize()
                t = di.parse_trace(capfd.readouterr().err)
                assert [v.instance for v in t] == [("two_pass",)] and t[0].radius == radius, t
                what = f"radius {radius}, 3 x {shape}, lut_in={lut}"
                _check(fused.cpu().numpy(), var, thr, what + ", fused")
                _check(two.cpu().numpy(), var, thr, what + ", two passes")
                assert torch.equal(fused, two)


@pytest.mark.parametrize("shape", PINNED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", RADII)
def test_variance_is_pinned(be, orc, radius, shape):
    import torch
    frames, var = _reference(orc, shape, False, radius)
    P = _palette(be, orc, False)
    d = np.unique(var)
    thrs = np.unique(np.concatenate([d, np.nextafter(d, np.float32(np.inf))])).astype(np.float32)
    assert len(thrs) >= len(d) + 1
    # what every call must give, by numpy's comparison (subnormal thresholds included), on the device as bytes
    want = torch.from_numpy((var[None] >= thrs[:, None, None, None]).astype(np.uint8)).cuda()
    x = torch.from_numpy(frames).cuda()
    bad = torch.zeros(len(thrs), dtype=torch.int64, device="cuda")
    for i, thr in enumerate(thrs):
        bad[i] = (be.variance_gate(x, P, float(thr), radius) != want[i]).sum()
    bad = bad.cpu().numpy()
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        got = be.variance_gate(x, P, float(thrs[i]), radius).cpu().numpy()
        _check(got, var, thrs[i], f"radius {radius}, 3 x {shape}: {int((bad > 0).sum())} of {len(thrs)} thresholds give a wrong map; the first")
        pytest.fail(f"radius {radius}, 3 x {shape}: threshold {float(thrs[i])!r} gave {bad[i]} wrong bytes once and none when repeated")


SUBNORMAL = float(np.nextafter(np.float32(0.0), np.float32(1.0)))
EDGES = (0.0, -0.0, -1.0, SUBNORMAL, float("inf"), float("nan"))


@pytest.mark.parametrize("radius", (0, 2))
def test_threshold_edges(be, orc, radius):
    import torch
    P = _palette(be, orc, False)
    for shape in PINNED_SHAPES:
        frames, var = _reference(orc, shape, False, radius)
        x = torch.from_numpy(frames).cuda()
        for thr in EDGES:
            got = be.variance_gate(x, P, thr, radius).cpu().numpy()
            _check(got, var, thr, f"radius {radius}, 3 x {shape}")
            if radius == 0 and thr == 0.0:          # (0.0 and -0.0)
                assert got.all()
            if radius == 0 and thr == SUBNORMAL:
                assert not got.any()
            if thr != thr or thr == float("inf"):
                assert not got.any()


def test_odd_input_address(be, orc):
    import torch
    radius, shape = 2, (17, 65)
    frames, var = _reference(orc, shape, False, radius)
    P = _palette(be, orc, False)
    A = ar.Arena(ar.capacity_for([(frames.size, ar.MIN_GUARD)]), device="cuda", seed=5)
    x = A.carve("in", frames.size, offset_mod16=1, guard=ar.MIN_GUARD).view(frames.shape)
    A.put("in", frames)
    assert x.data_ptr() % 2 == 1
    for thr in _some_thresholds(var):
        _check(be.variance_gate(x, P, float(thr), radius).cpu().numpy(), var, thr, f"radius {radius}, 3 x {shape} at an odd address")
    A.check()
    A.unchanged("in")
