"""GPU tier of the address arithmetic of the fine kernel's main loop (dither_pie_amd/csrc/ordered.hip: ordered_fine_kernel<1, 1, 2>;
ordered_fine.h: fine_cell_offset, fine_stage_tag, fine_row_offset).  SUB 2 stages `off` at the start of LDS and the rows behind it, a
wide cell's tag as the offset of its row, and tests the window numbers as 32-bit values: none of that may change a byte.  The product
library and the experiments twin (whose trace must say `keys=1 sub=2`), Bayer 8x8, palr(256, 7), byte for byte against the CPU oracle.

Shapes: three frames of width 1021 -- groups of four pixels straddle row ends -- and a height such that the 4096-pixel tiles number
C + 1, 2C + 2 and 3C + 10 for the device's C compute units: the persistent workgroups make 1-2, 2-3 and 3-4 trips of the main loop, an
odd and an even number of them side by side.  Contents: the first rows hold every colour of the sixteen wide cells of highest rank (the
longest row offsets a tag can hold) and every colour of the sub-cells that are still wide (row entry 0: the deferred path decodes the
tag), from tests/golden/fine_sub_palr256_7.npz; the rest is seeded noise.  One oracle pass per shape, shared by both libraries.
The CPU side: tests/test_ordered_fine_addr_cpu.py."""
import re

import numpy as np
import pytest

import fine_sub_ref as fs

pytestmark = pytest.mark.gpu

W, FRAMES, TILE = 1021, 3, 4096
TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) .* kernel=(\w+) keys=(\d) sub=(\d)")
TILES = pytest.mark.parametrize("tiles", ["C+1", "2C+2", "3C+10"])
_CASES = {}   # tiles -> (frames, oracle output): made once, never written again


def _n_tiles(name):
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    c = torch.cuda.get_device_properties(0).multi_processor_count
    return {"C+1": c + 1, "2C+2": 2 * c + 2, "3C+10": 3 * c + 10}[name]


def _height(n_tiles):
    """the height at which FRAMES frames of width W make exactly n_tiles tiles (a tile is wider than a row of all the frames)"""
    h = -(-((n_tiles - 1) * TILE + 1) // (FRAMES * W))
    assert (n_tiles - 1) * TILE < FRAMES * h * W <= n_tiles * TILE
    return h


def _contents(n, seed):
    fx = np.load(fs.FIXTURE)
    cells = fx["wide_cell"].astype(np.int64)
    head = [fs.colours(int(c)) for c in cells[-16:]]
    head += [fs.colours(int(cells[int(s) >> 3]), int(s) & 7) for s in fx["sub_wide"]]
    head = np.concatenate(head).astype(np.uint8)
    assert len(head) == 16 * 512 + 64 * len(fx["sub_wide"]) <= n
    noise = np.random.RandomState(seed).randint(0, 256, (n - len(head), 3)).astype(np.uint8)
    return np.concatenate([head, noise])


def _case(orc, name):
    if name not in _CASES:
        t = _n_tiles(name)
        h = _height(t)
        arr = _contents(FRAMES * h * W, 30 + len(name)).reshape(FRAMES, h, W, 3)
        pal_f32, out_colors, lut_in = orc.prepare_palette(orc.palr(256, 7), False)
        thr = orc.bayer_matrix("8x8")
        ref = np.stack([orc.ordered_u8(f, pal_f32, out_colors, lut_in, "matrix", thr=thr) for f in arr])
        arr.setflags(write=False)
        ref.setflags(write=False)
        _CASES[name] = (arr, ref)
    return _CASES[name]


def _check(be, orc, name):
    import torch
    arr, ref = _case(orc, name)
    pal_f32, out_colors, lut_in = orc.prepare_palette(orc.palr(256, 7), False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    out = be.ordered(torch.tensor(arr).cuda(), P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(orc.bayer_matrix("8x8"))).cpu().numpy()
    bad = np.argwhere((out != ref).any(-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}"


@TILES
def test_product_library(orc, tiles):
    from dither_pie_amd import backend
    _check(backend, orc, tiles)


@TILES
def test_experiments_twin_at_sub_2(orc, switches, capfd, tiles):
    switches.setenv("DP_ORDERED_TRACE", "1")
    switches.setenv("DP_FINE_SUB_MAX", "2")
    from dither_pie_amd import backend
    capfd.readouterr()
    _check(backend, orc, tiles)
    seen = TRACE.findall(capfd.readouterr().err)
    assert seen == [("lean", "fine", "1", "2")], seen
