"""GPU tier of ordered_fine_kernel (dither_pie_amd/csrc/ordered.hip): the lean kernel's main loop on candidate windows of 4 + 2
entries shared by the 32^3 cells of 8 colours a side.  Bytes equal to the CPU oracle, and in every case the trace line of the
experiments library must say that the fine kernel was the one launched (`kernel=fine` behind the plan it replaces):
  * all 2^24 colours as one 4096 x 4096 frame, palr(256,7), Bayer 8x8: every cell, every wide cell, every tie;
  * 258 x 19 (groups that straddle a row end, a partial last group) and 256 x 16 (exactly one tile);
  * a row band at (y0, 0) through sharding.dither_band and a frame at a non-zero (y0, x0);
  * 512 x 512 with a 16 x 16 integer matrix whose slots mix both sides of 1/2: no classes, every slot is a full slot;
  * the library that ships gives the same bytes (it has no trace to read).
The CPU side of the table and of the choice: tests/test_ordered_fine_cpu.py."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) .* kernel=(\w+)")


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


def _fine(switches):
    switches.setenv("DP_ORDERED_TRACE", "1")
    from dither_pie_amd import backend
    return backend


def _launched_fine(capfd, launches=1):
    seen = TRACE.findall(capfd.readouterr().err)
    assert seen == [("lean", "fine")] * launches, seen


def _case(be, orc, capfd, arr, thr, y0=0, x0=0, pal=None):
    pal = pal or orc.palr(256, 7)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    if capfd is not None:
        capfd.readouterr()
    out = be.ordered(_dev(arr), P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(thr), y0=y0, x0=x0).cpu().numpy()
    if capfd is not None:
        _launched_fine(capfd)
    ref = orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=thr, y0=y0, x0=x0)
    bad = np.argwhere((out != ref).any(-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}"


def test_every_colour_bayer8(orc, switches, capfd):
    v = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
    _case(_fine(switches), orc, capfd, cube, orc.bayer_matrix("8x8"))


@pytest.mark.parametrize("h,w,seed", [(19, 258, 3), (16, 256, 4)], ids=["258x19-straddling-rows", "256x16-one-tile"])
def test_small_frames_bayer8(orc, switches, capfd, h, w, seed):
    _case(_fine(switches), orc, capfd, orc.rnd(h, w, seed), orc.bayer_matrix("8x8"))


def test_origin_and_row_band(orc, switches, capfd):
    import torch
    be = _fine(switches)
    _case(be, orc, capfd, orc.rnd(37, 130, 6), orc.bayer_matrix("8x8"), y0=5, x0=3)
    from dither_pie_amd import dithering_lib as dl, sharding
    pal = orc.palr(256, 7)
    img = orc.rnd(61, 203, 8)
    d = dl.ImageDitherer(256, dl.DitherMode.BAYER, pal, False, {"size": "8x8"}).prepare()    # (with the accelerator, as a video job has it)
    capfd.readouterr()
    bands = [sharding.dither_band(d, _dev(img[lo:hi]), lo) for lo, hi in ((0, 21), (21, 22), (22, 61))]
    _launched_fine(capfd, 3)
    assert np.array_equal(torch.cat(bands).cpu().numpy(), orc.apply_dithering(img, pal, "bayer", {"size": "8x8"}))


def test_matrix_without_classes(orc, switches, capfd):
    _case(_fine(switches), orc, capfd, orc.rnd(512, 512, 9), _mixed16())


def test_product_library(orc):
    from dither_pie_amd import backend
    _case(backend, orc, None, orc.rnd(130, 258, 10), orc.bayer_matrix("8x8"))
    _case(backend, orc, None, orc.rnd(64, 67, 11), orc.bayer_matrix("8x8"), pal=orc.palr(256, 11))
