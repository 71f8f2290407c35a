"""GPU tier of the key levels of ordered_fine_kernel (dither_pie_amd/csrc/ordered.hip; ordered_fine.h: fine_keys_level): at levels 1
and 2 the kernel builds arrays of colours and of their norms in LDS from the unchanged table image, forms a candidate key with two instructions
(cand4k / cand6k), and reads the flat lists of the wide cells from global memory.  Every key value is today's, so the bytes must be:
  * levels 1 and 2 (DP_FINE_KEYS_MAX of the experiments library) on 258 x 19 (groups that straddle a row end, a partial last group) and
    256 x 16 (exactly one tile), palr(256,7), Bayer 8x8: equal to the CPU oracle, and the trace says `kernel=fine keys=<level>`;
  * a 16 x 16 matrix whose slots mix both sides of 1/2 (no classes: every slot is a full slot, cand6k everywhere) on 256 x 64;
  * all 2^24 colours as one 4096 x 4096 frame at levels 1 and 2: equal ON THE DEVICE to the level-0 output of the same library -- every
    window, every wide cell through the global lists, every tie, 16 tiles per workgroup through the two-tile prefetch;
  * a frame at a non-zero (y0, x0), level 2;
  * the product library has no switch and takes the level by budget, up to the one that measured fastest (ordered_fine.h:
    kFineKeysShipped; the level-2 instance exists in the experiments build only): palr(256,11) against the oracle.
The CPU side (the choice of the level, the key identity): tests/test_ordered_fine_keys_cpu.py."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) .* kernel=(\w+) keys=(\d)")


def _dev(a):
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mixed16():
    """16 x 16 thresholds m / 256: the four columns a pixel slot of a wave meets in a row (x, x + 4, x + 8, x + 12) hold
    values from all four quarters of [0, 1), so no slot is nearest-only and the table has no classes."""
    y, x = np.mgrid[0:16, 0:16]
    m = 64 * ((x // 4 + y) % 4) + 16 * (x % 4) + (5 * y + 3 * x) % 16
    assert all(len({int(v) // 128 for v in m[r, c::4]}) == 2 for r in range(16) for c in range(4))
    return (m / 256.0).astype(np.float32)


def _at_level(switches, level):
    switches.setenv("DP_ORDERED_TRACE", "1")
    switches.setenv("DP_FINE_KEYS_MAX", str(level))
    from dither_pie_amd import backend
    return backend


def _launched(capfd, level):
    seen = TRACE.findall(capfd.readouterr().err)
    assert seen == [("lean", "fine", str(level))], seen


def _run(be, orc, capfd, level, arr_dev, thr, y0=0, x0=0, pal=None):
    pal = pal or orc.palr(256, 7)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    if capfd is not None:
        capfd.readouterr()
    out = be.ordered(arr_dev, P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(thr), y0=y0, x0=x0)
    if capfd is not None:
        _launched(capfd, level)
    return out


def _case(be, orc, capfd, level, arr, thr, y0=0, x0=0, pal=None):
    out = _run(be, orc, capfd, level, _dev(arr), thr, y0, x0, pal).cpu().numpy()
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal or orc.palr(256, 7), False)
    ref = orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=thr, y0=y0, x0=x0)
    bad = np.argwhere((out != ref).any(-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}"


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("h,w,seed", [(19, 258, 3), (16, 256, 4)], ids=["258x19-straddling-rows", "256x16-one-tile"])
def test_small_frames_bayer8(orc, switches, capfd, h, w, seed, level):
    _case(_at_level(switches, level), orc, capfd, level, orc.rnd(h, w, seed), orc.bayer_matrix("8x8"))


@pytest.mark.parametrize("level", [1, 2])
def test_matrix_without_classes(orc, switches, capfd, level):
    _case(_at_level(switches, level), orc, capfd, level, orc.rnd(64, 256, 9), _mixed16())


_CUBE = {}   # the 4096 x 4096 frame of all colours and its level-0 output, on the device: made once, never written again


def _cube_level0(orc, switches, capfd):
    if not _CUBE:
        import torch
        v = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
        cube = torch.stack([v & 255, (v >> 8) & 255, v >> 16], -1).to(torch.uint8).reshape(4096, 4096, 3).contiguous()
        out0 = _run(_at_level(switches, 0), orc, capfd, 0, cube, orc.bayer_matrix("8x8")).clone()
        _CUBE.update(cube=cube, out0=out0)
    return _CUBE["cube"], _CUBE["out0"]


@pytest.mark.parametrize("level", [1, 2])
def test_every_colour_equals_level0(orc, switches, capfd, level):
    import torch
    cube, out0 = _cube_level0(orc, switches, capfd)
    out = _run(_at_level(switches, level), orc, capfd, level, cube, orc.bayer_matrix("8x8"))
    if not torch.equal(out, out0):
        bad = torch.nonzero((out != out0).any(-1))
        raise AssertionError(f"{len(bad)} pixels differ from level 0, first at {bad[:4].tolist()}")


def test_origin_level2(orc, switches, capfd):
    _case(_at_level(switches, 2), orc, capfd, 2, orc.rnd(37, 130, 6), orc.bayer_matrix("8x8"), y0=5, x0=3)


def test_product_library_by_budget(orc):
    from dither_pie_amd import backend
    _case(backend, orc, None, None, orc.rnd(67, 64, 11), orc.bayer_matrix("8x8"), pal=orc.palr(256, 11))
