"""GPU tier of the one-launch path of the ordered dither (dither_pie_amd/csrc/ordered_fix.h: fix_needed; ordered.hip: launch_ordered and
the NOFLAGS instances of ordered_fine_kernel): where the palette can never flag a pixel, a call is the pass-1 kernel alone -- no reset of
the flagged-tile count, no fix-up launch, and the fine kernel does not clear the flag bitmap.  The bytes are what they were:
  (a) palr(256,7), Bayer 8x8 against the CPU oracle on 16 x 256 (exactly one tile), 19 x 257 (a partial last group, groups that straddle a
      row end) and 1040 x 1024 at a non-zero origin (more tiles than workgroups); the trace says `kernel=fine ... fix=0`, and a workspace
      of exactly dp_ordered_workspace_bytes filled with 0xA5 is byte-identical after the call: the path writes nothing to it;
  (b) all 2^24 colours as one 4096 x 4096 frame, Bayer 8x8 (the fine kernel, the k = 2 tie codes) and mode `none` (the lean kernel, the
      k = 1 codes; DP_NO_FAST keeps the fast kernel away): the one-launch output equals the output under DP_ALWAYS_FIXUP=1 byte for byte
      -- a wrong fix_needed leaves a flagged pixel unrepaired, and this comparison sees it;
  (c) a palette that must keep the pass: twelve colours at squared distance 25 from (128,128,128) and no other within 64, so that the
      centre's candidates exceed a block; the trace says fix=1 and a noise frame with the centre sown in equals the oracle;
  (d) Bayer 4x4, 16 uniform colours, 2 frames of 64 x 256 (the video leg's launch in small): equal to the oracle, and the traced fix= is
      what tests/ordered_fix_ref.py says for the facts the accelerator build reports (DP_DEBUG_ACCEL).
The CPU side (the decision function): tests/test_ordered_fix_needed_cpu.py."""
import re

import numpy as np
import pytest

import ordered_fix_ref as fx

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) .* table=(\w+) .* kernel=(\w+).* fix=(\d)")
FACTS = re.compile(r"fix-up facts: slow_blocks=(-?\d+) warp_slow_blocks=(-?\d+) n_exc=(-?\d+)")


def _dev(a):
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _traced(switches):
    switches.setenv("DP_ORDERED_TRACE", "1")
    from dither_pie_amd import backend
    return backend


def _palette(be, orc, pal):
    return be.Palette(*orc.prepare_palette(pal, False), accel=True)


def _differences(out, ref, arr):
    bad = np.argwhere((out != ref).any(-1))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}"


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,seed,y0,x0", [(16, 256, 4, 0, 0), (19, 257, 3, 0, 0), (1040, 1024, 8, 5, 3)],
                         ids=["256x16-one-tile", "257x19-straddling-rows", "1024x1040-origin"])
def test_fine_kernel_alone_and_workspace_untouched(orc, switches, capfd, h, w, seed, y0, x0):
    import torch
    from dither_pie_amd import _lib
    be = _traced(switches)
    arr, pal, thr = orc.rnd(h, w, seed), orc.palr(256, 7), orc.bayer_matrix("8x8")
    P, T = _palette(be, orc, pal), be.Thresholds.from_matrix(thr)
    L = _lib.load()
    need = int(L.dp_ordered_workspace_bytes(1, h, w))
    x = _dev(arr)
    out = torch.full_like(x, 0x5A)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    capfd.readouterr()
    _lib.check(L.dp_ordered_u8(x.data_ptr(), out.data_ptr(), 1, h, w, y0, x0, P._h, be.MODE_MATRIX, T._h, 1.0, 0, ws.data_ptr(), need,
                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    seen = TRACE.findall(capfd.readouterr().err)
    assert seen == [("lean", "plain8", "fine", "0")], seen
    assert bool((ws == 0xA5).all()), "the one-launch path wrote to the workspace"
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    _differences(out.cpu().numpy(), orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=thr, y0=y0, x0=x0), arr)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
_CUBE = {}   # the 4096 x 4096 frame of all colours, on the device: made once, never written again


def _cube():
    if not _CUBE:
        import torch
        v = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
        _CUBE["cube"] = torch.stack([v & 255, (v >> 8) & 255, v >> 16], -1).to(torch.uint8).reshape(4096, 4096, 3).contiguous()
    return _CUBE["cube"]


@pytest.mark.parametrize("mode,kernel", [("matrix", "fine"), ("none", "lean")], ids=["bayer8-fine-k2", "none-lean-k1"])
def test_every_colour_equals_the_three_dispatches(orc, switches, capfd, mode, kernel):
    import torch
    be = _traced(switches)
    switches.setenv("DP_NO_FAST", "1")   # (read when the accelerator is built: mode `none` then stays on the lean kernel)
    P = _palette(be, orc, orc.palr(256, 7))
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("8x8")) if mode == "matrix" else None
    m = be.MODE_MATRIX if mode == "matrix" else be.MODE_NEAREST
    cube = _cube()
    capfd.readouterr()
    one = be.ordered(cube, P, m, thr=thr).clone()
    switches.setenv("DP_ALWAYS_FIXUP", "1")
    three = be.ordered(cube, P, m, thr=thr)
    torch.cuda.synchronize()
    seen = [(k, f) for _, _, k, f in TRACE.findall(capfd.readouterr().err)]
    assert seen == [(kernel, "0"), (kernel, "1")], seen
    if not torch.equal(one, three):
        bad = torch.nonzero((one != three).any(-1))
        raise AssertionError(f"{len(bad)} pixels differ between one launch and three, first at {bad[:4].tolist()}")


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def _ring_palette(orc):
    c = 128
    ring = ([(c + a, c + b, c) for a in (-3, 3) for b in (-4, 4)] + [(c + a, c + b, c) for a in (-4, 4) for b in (-3, 3)] +
            [(c, c + a, c + b) for a in (-3, 3) for b in (-4, 4)])
    rest = [p for p in orc.palr(100, 5) if sum((v - c) ** 2 for v in p) > 64]
    return ring + rest


def test_palette_with_a_slow_block_keeps_the_pass(orc, switches, capfd):
    be = _traced(switches)
    pal = _ring_palette(orc)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    # brute force: the centre has twelve nearest entries at squared distance 25 and nothing else within 64 -- more than a block holds
    d = ((np.asarray(pal_f32, np.float64) - 128.0) ** 2).sum(-1)
    assert len(set(pal)) == len(pal) and d.min() == 25.0 and int((d == 25.0).sum()) == 12 and int((d <= 64.0).sum()) == 12
    arr = orc.rnd(64, 256, 21).copy()
    sow = np.random.RandomState(22).rand(64, 256) < 0.01
    arr[sow] = 128
    assert 100 < int(sow.sum()) < 260
    thr = orc.bayer_matrix("8x8")
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    capfd.readouterr()
    out = be.ordered(_dev(arr), P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(thr)).cpu().numpy()
    seen = TRACE.findall(capfd.readouterr().err)
    assert len(seen) == 1 and seen[0][3] == "1", seen
    _differences(out, orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=thr), arr)


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_video_launch_shape_in_small(orc, switches, capfd):
    be = _traced(switches)
    switches.setenv("DP_DEBUG_ACCEL", "1")
    pal = orc.generate_uniform_palette(16)
    pal_f32, out_colors, lut_in = orc.prepare_palette(pal, False)
    thr = orc.bayer_matrix("4x4")
    frames = np.stack([orc.rnd(64, 256, 31), orc.rnd(64, 256, 32)])
    capfd.readouterr()
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    out = be.ordered(_dev(frames), P, be.MODE_MATRIX, thr=be.Thresholds.from_matrix(thr)).cpu().numpy()
    err = capfd.readouterr().err
    seen, facts = TRACE.findall(err), FACTS.findall(err)
    assert len(seen) == 1 and len(facts) == 1, (seen, facts)
    family, table, kernel, fix = seen[0]
    slow, warp_slow, n_exc = (int(v) for v in facts[0])
    want = fx.fix_needed(dict(family=family, fine=int(kernel == "fine"), is_integer=1, accel=1, table=table,
                              slow_blocks={"plain8": slow, "plain4": 0, "warped": warp_slow}[table], n_exc=n_exc), dict(always_fixup=0))
    assert int(fix) == int(want), (seen, facts)
    for i in range(2):
        _differences(out[i], orc.ordered_u8(frames[i], pal_f32, out_colors, lut_in, "matrix", thr=thr), frames[i])
