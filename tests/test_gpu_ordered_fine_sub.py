"""GPU tier of the two-level fine table (dither_pie_amd/csrc/ordered.hip: ordered_fine_kernel<1, 1, SUB>; ordered_fine.h: fine_sub_level).
SUB 2: the main loop replaces the tag of a wide cell by the window of the pixel's 4-wide sub-cell, one tile ahead, and only the pixels
of sub-cells that are still wide are deferred for their set's sake.  SUB 1 (experiments build only): the main loop is today's and the
deferred path ranks a wide cell's pixel on its sub-cell's window in LDS.  A sub-cell's window holds its N in the quad and its T in the
six, as a cell's does, so every byte must be what it was.  palr(256,7) and Bayer 8x8 unless said; both levels, set with DP_FINE_SUB_MAX
of the experiments library, and the trace must say `keys=1 sub=<n>`:
  * frames whose colours come from wide cells only (tests/golden/fine_sub_palr256_7.npz: all eight sub-cells of every wide cell, the
    still-wide ones among them), 256 x 64 -- every lane of every slot takes the lookup -- and 258 x 19 -- groups that straddle a row end,
    a partial last group -- against the CPU oracle; the 256 x 64 one also under a 16 x 16 matrix without classes (every slot a full one);
  * rnd(19, 258) and rnd(16, 256): exactly one tile, nothing to look up ahead for;
  * pipeline tails: (k - 1) * n_cus + 1 tiles of 1024 pixels plus 7 pixels, k = 1..4, so that workgroups walk from 1 to 4 tiles and the
    last tile is a partial one (h x 1024 has no 7 pixels over: the frame is one row);
  * a non-zero (y0, x0) on 130 x 37;
  * all 2^24 colours as one 4096 x 4096 frame: equal ON THE DEVICE to the level-0 output of the same library -- every window, every
    row, every tie, 16 tiles per workgroup;
  * DP_FINE_SUB_MAX=0 launches today's kernel (`sub=0`), same bytes;
  * the product library with nothing forced, palr(256,11) on 64 x 67.
The CPU side: tests/test_ordered_fine_sub_cpu.py."""
import re

import numpy as np
import pytest

import fine_sub_ref as fs

pytestmark = pytest.mark.gpu

SUBS = pytest.mark.parametrize("sub", [1, 2])
TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) .* kernel=(\w+) keys=(\d) sub=(\d)")


def _dev(a):
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mixed16():
    """16 x 16 thresholds m / 256 (as in test_gpu_ordered_fine_keys.py): the four columns a pixel slot of a wave meets in a row hold
    values from both sides of 1/2, so no slot is nearest-only and the table has no classes."""
    y, x = np.mgrid[0:16, 0:16]
    m = 64 * ((x // 4 + y) % 4) + 16 * (x % 4) + (5 * y + 3 * x) % 16
    assert all(len({int(v) // 128 for v in m[r, c::4]}) == 2 for r in range(16) for c in range(4))
    return (m / 256.0).astype(np.float32)


def _at_sub(switches, sub, keys=None):
    switches.setenv("DP_ORDERED_TRACE", "1")
    switches.setenv("DP_FINE_SUB_MAX", str(sub))
    if keys is not None:
        switches.setenv("DP_FINE_KEYS_MAX", str(keys))
    from dither_pie_amd import backend
    return backend


def _run(be, orc, capfd, want, arr_dev, thr, y0=0, x0=0, pal=None):
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal or orc.palr(256, 7), False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    if capfd is not None:
        capfd.readouterr()
    out = be.ordered(arr_dev, P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(thr), y0=y0, x0=x0)
    if capfd is not None:
        seen = TRACE.findall(capfd.readouterr().err)
        assert seen == [("lean", "fine", str(want[0]), str(want[1]))], seen
    return out


def _case(be, orc, capfd, want, arr, thr, y0=0, x0=0, pal=None):
    out = _run(be, orc, capfd, want, _dev(arr), thr, y0, x0, pal).cpu().numpy()
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal or orc.palr(256, 7), False)
    ref = orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=thr, y0=y0, x0=x0)
    bad = np.argwhere((out != ref).any(-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}"


@SUBS
@pytest.mark.parametrize("h,w,seed", [(64, 256, 1), (19, 258, 2)], ids=["256x64-four-tiles", "258x19-straddling-rows"])
def test_wide_only_frames(orc, switches, capfd, h, w, seed, sub):
    arr = fs.wide_only_colours(h * w, seed).reshape(h, w, 3)
    _case(_at_sub(switches, sub), orc, capfd, (1, sub), arr, orc.bayer_matrix("8x8"))


@SUBS
def test_wide_only_matrix_without_classes(orc, switches, capfd, sub):
    arr = fs.wide_only_colours(64 * 256, 1).reshape(64, 256, 3)
    _case(_at_sub(switches, sub), orc, capfd, (1, sub), arr, _mixed16())


@SUBS
@pytest.mark.parametrize("h,w,seed", [(19, 258, 3), (16, 256, 4)], ids=["258x19", "256x16-one-tile"])
def test_small_random_frames(orc, switches, capfd, h, w, seed, sub):
    _case(_at_sub(switches, sub), orc, capfd, (1, sub), orc.rnd(h, w, seed), orc.bayer_matrix("8x8"))


@SUBS
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_pipeline_tails(orc, switches, capfd, k, sub):
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    w = ((k - 1) * n_cus + 1) * 1024 + 7
    _case(_at_sub(switches, sub), orc, capfd, (1, sub), orc.rnd(1, w, 20 + k), orc.bayer_matrix("8x8"))


@SUBS
def test_origin(orc, switches, capfd, sub):
    _case(_at_sub(switches, sub), orc, capfd, (1, sub), orc.rnd(37, 130, 6), orc.bayer_matrix("8x8"), y0=5, x0=3)


_CUBE = {}   # the 4096 x 4096 frame of all colours and its level-0 output, on the device: made once, never written again


@SUBS
def test_every_colour_equals_level0(orc, switches, capfd, sub):
    import torch
    if not _CUBE:
        v = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
        cube = torch.stack([v & 255, (v >> 8) & 255, v >> 16], -1).to(torch.uint8).reshape(4096, 4096, 3).contiguous()
        out0 = _run(_at_sub(switches, 0, keys=0), orc, capfd, (0, 0), cube, orc.bayer_matrix("8x8")).clone()
        switches.delenv("DP_FINE_KEYS_MAX")
        _CUBE.update(cube=cube, out0=out0)
    cube, out0 = _CUBE["cube"], _CUBE["out0"]
    out = _run(_at_sub(switches, sub), orc, capfd, (1, sub), cube, orc.bayer_matrix("8x8"))
    if not torch.equal(out, out0):
        bad = torch.nonzero((out != out0).any(-1))
        raise AssertionError(f"{len(bad)} pixels differ from level 0, first at {bad[:4].tolist()}")


def test_sub_max_0_is_todays_kernel(orc, switches, capfd):
    _case(_at_sub(switches, 0), orc, capfd, (1, 0), fs.wide_only_colours(19 * 258, 2).reshape(19, 258, 3), orc.bayer_matrix("8x8"))


def test_product_library_nothing_forced(orc):
    from dither_pie_amd import backend
    _case(backend, orc, None, None, orc.rnd(67, 64, 11), orc.bayer_matrix("8x8"), pal=orc.palr(256, 11))
