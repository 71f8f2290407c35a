"""GPU tier: the second and later groups of the launchers that split a batch and re-use their workspace.

launch_wavelet and launch_halftone process frames in groups bounded by scratch bytes and by 65535 grid rows; the variance
gate's fused path goes in groups of 65535 frames; Riemersma takes frames on grid.x.  The value tests never give them more
than one group.  Here every batch needs several, through the product path (dl.*Strategy.dither_frames / backend.*): the
byte-bounded cases assert through the size queries that the batch really is split, and every frame of every batch is
compared -- with the CPU restatement, or (4K wavelet) with the single-frame call and the reference's recorded hash.

The launchers of pattern dithering, dot diffusion, cell palettes, the Oklab ordered kernel and integer error diffusion loop
over groups of 65535 frames as well and re-derive their input, output, `sets` and workspace pointers per group: each gets
65535 + 7 frames here, against its statement (pattern_ref, dotdiff_ref, cells_ref, metric_ref, idiff_ref).  The `sets` plane
of the cells and the workspace of the integer diffusion (32 w bytes per frame, the one of these with a per-frame workspace)
are carved from a guarded arena (tests/arena.py) at exactly their size, so a group that starts at the wrong offset either
shows in a frame or in a guard.  dp_ordered_u8 (the RGB ordered kernel) had no test with more than 65535 frames either; it
splits by pixels, not by frames (2^30 per launch), and gets the same batch.

Grid-bounded batches repeat 64 distinct frames (the group sizes are not multiples of 64, so a whole-group offset error
cannot map a frame onto an equal one)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import arena as ar
import cells_ref
import dotdiff_ref
import halftone_ref
import idiff_ref
import metric_ref
import pattern_ref
import riemersma_ref
import wavelet_ref as wr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "wavelet.json")) as _fh:
    WL = json.load(_fh)
PERIOD = 64


@pytest.fixture(scope="module")
def dl():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import dithering_lib
    return dithering_lib


def _need_memory(nbytes):
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"not enough free HBM ({free >> 20} MiB, {nbytes >> 20} MiB needed)")


def _base(orc, h, w, seed):
    """PERIOD distinct frames; a batch of n repeats them: _tile(base, n)[k] is base[k % PERIOD]."""
    return np.stack([orc.rnd(h, w, seed + k) for k in range(PERIOD)])


def _tile(base, n):
    return base[np.arange(n) % PERIOD]


def _assert_every_frame(got, refs, what):
    """got [n, ...] on the host, refs [PERIOD, ...]: frame k must equal refs[k % PERIOD]."""
    n = got.shape[0]
    want = _tile(refs, n)
    bad = np.nonzero((got.reshape(n, -1) != want.reshape(n, -1)).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {n} frames differ, first {bad[:8].tolist()}"


# ------------------------------------------------------------------------------------------------ wavelet
def test_wavelet_4k_batch_in_groups_bounded_by_bytes(dl, orc):
    """5 frames of 2160 x 3840, haar: about 232 MB of scratch per frame, so the 512 MB bound gives groups of 2, 2, 1."""
    import torch
    from dither_pie_amd import _lib, backend
    h, w, n = 2160, 3840, 5
    case = next(c for c in WL["cases"] if c["name"] == "wl_2160x3840_p16")
    assert case["params"] == {} and not case["use_gamma"] and (case["h"], case["w"]) == (h, w)
    n0, n1 = (h + 1) // 2, (w + 1) // 2
    per = 256 + 4 * (6 * n0 * w + 12 * n0 * n1 + h * w)
    P = backend.WaveletParams(0, 8, None, 0)
    L = _lib.load()
    assert L.dp_wavelet_workspace_bytes(1, h, w, C.byref(P)) == per
    assert L.dp_wavelet_workspace_bytes(n, h, w, C.byref(P)) == 2 * per           # G = 2: three groups for five frames
    _need_memory(2 * n * h * w * 3 + 2 * per + (1 << 30))
    pal = [tuple(c) for c in case["palette"]]
    fixture = wr.make_input(case["input"])
    assert hashlib.sha256(fixture.tobytes()).hexdigest() == case["input_sha256"]
    frames = [orc.rnd(h, w, 71), orc.imgl(h, w, 72), fixture, orc.rnd(h, w, 73), fixture]
    frames[3][..., 1] = 99                                                        # a flat channel in the second group
    x = torch.from_numpy(np.stack(frames)).cuda()
    s = dl.WaveletDitherStrategy()
    batch = s.dither_frames(x, pal, False)
    for k in range(n):
        one = s.dither_frames(x[k], pal, False)
        assert torch.equal(batch[k], one), f"frame {k} of the batch differs from its single-frame call"
    for k in (2, 4):
        assert hashlib.sha256(batch[k].cpu().numpy().tobytes()).hexdigest() == case["output_sha256"], k
    del x, batch
    torch.cuda.empty_cache()


@pytest.mark.parametrize("h,w", [(2, 3), (1, 1)])
def test_wavelet_batch_in_groups_bounded_by_the_grid(dl, orc, h, w):
    """65535 // 3 + 7 frames: the second group is seven frames long."""
    import torch
    n = 65535 // 3 + 7
    assert (65535 // 3) % PERIOD != 0
    pal = orc.palr(16, 3)
    base = _base(orc, h, w, 500)
    base[5] = base[5][:1, :1]                                                       # a flat frame among them
    frames = _tile(base, n)
    refs = np.stack([wr.apply(f, pal, False, WL["taps"]) for f in base])
    got = dl.WaveletDitherStrategy().dither_frames(torch.from_numpy(frames).cuda(), pal, False).cpu().numpy()
    _assert_every_frame(got, refs, f"wavelet {n} x {h}x{w}")


# ------------------------------------------------------------------------------------------------ halftone
@pytest.mark.parametrize("K,params", [(16, {}), (300, {}), (16, {"dot_gain": 1.5})], ids=["K16", "K300-ties", "K16-pow"])
def test_halftone_1080p_batch_in_groups_bounded_by_bytes(dl, orc, K, params):
    """5 frames of 1080 x 1920 with one-pixel cells at 45 degrees: millions of cells per frame, groups of 2, 2, 1."""
    import torch
    from dither_pie_amd import _lib, backend
    h, w, n = 1080, 1920, 5
    full = dict(halftone_ref.DEFAULTS, cell_size=1, angle=45.0, **params)
    pal = orc.palr(K, 5)
    if K == 300:
        pal = pal[:150] + pal[:150]                                               # duplicated entries: exact ties, the tie kernel
    L = _lib.load()
    hp = backend.halftone_params(np.asarray(pal, np.float32), **full)
    need = [L.dp_halftone_workspace_bytes(k, h, w, C.byref(hp)) for k in (1, 2, 3, 5)]
    per = need[1] - need[0]
    assert per > 0 and per % 20 == 0                                              # 20 bytes per cell
    assert need[2] == need[1] and need[3] == need[1]                            # G = 2 whatever the batch: 2, 2, 1 for five frames
    _need_memory(2 * n * h * w * 3 + need[3] + (1 << 30))
    frames = np.stack([orc.rnd(h, w, 80), orc.imgl(h, w, 81), orc.rnd(h, w, 82), orc.imgl(h, w, 83, "dark"), orc.rnd(h, w, 84)])
    got = dl.HalftoneDitherStrategy(**full).dither_frames(torch.from_numpy(frames).cuda(), pal, False).cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], halftone_ref.apply(frames[k], pal, False, **full)), f"frame {k}"
    torch.cuda.empty_cache()


def test_halftone_batch_in_groups_bounded_by_the_grid(dl, orc):
    import torch
    n, h, w = 65535 + 7, 2, 3
    assert 65535 % PERIOD != 0
    pal = orc.palr(16, 4)
    base = _base(orc, h, w, 600)
    frames = _tile(base, n)
    refs = np.stack([halftone_ref.apply(f, pal, False, **halftone_ref.DEFAULTS) for f in base])
    got = dl.HalftoneDitherStrategy().dither_frames(torch.from_numpy(frames).cuda(), pal, False).cpu().numpy()
    _assert_every_frame(got, refs, f"halftone {n} x {h}x{w}")


# ------------------------------------------------------------------------------------------------ gate, riemersma
@pytest.mark.parametrize("h,w", [(3, 3), (5, 2)])
def test_variance_gate_fused_path_in_groups_of_65535_frames(orc, h, w):
    import torch
    from dither_pie_amd import backend
    n = 65535 + 7
    base = _base(orc, h, w, 700)
    base[9] = 128
    frames = _tile(base, n)
    P = backend.Palette(*orc.prepare_palette(orc.palr(16), False))
    refs = np.stack([orc.variance_gate(f, 300.0, 1)[0] for f in base])
    assert 0 < refs.mean() < 1                                                    # both gate values occur
    got = backend.variance_gate(torch.from_numpy(frames).cuda(), P, 300.0, 1).cpu().numpy()
    _assert_every_frame(got, refs, f"variance gate {n} x {h}x{w}")


def test_riemersma_seventy_thousand_frames(orc):
    """No split, but frames go on grid.x: nothing may assume a 16-bit frame index."""
    import torch
    from dither_pie_amd import backend
    n, h, w = 70000, 2, 2
    pal = [(0, 0, 0), (255, 255, 255)]
    base = _base(orc, h, w, 800)
    frames = _tile(base, n)
    refs = np.stack([riemersma_ref.apply(f, pal, False) for f in base])
    P = backend.Palette(*orc.prepare_palette(pal, False))
    got = backend.riemersma(torch.from_numpy(frames).cuda(), P).cpu().numpy()
    _assert_every_frame(got, refs, f"riemersma {n} x {h}x{w}")


# ------------------------------------------------------------------------------------------------ the table kernels
N_TABLE = 65535 + 7
MODE_NEAREST, MODE_MATRIX = 0, 1


def _table_palette(orc, seed):
    from dither_pie_amd import backend
    spec = orc.prepare_palette(orc.palr(16, seed), False)
    return spec, backend.Palette(*spec)


@pytest.mark.parametrize("matrix,y0,x0", [(4, 1, 2), (8, 0, 0)])
def test_pattern_in_groups_of_65535_frames(orc, matrix, y0, x0):
    import torch
    from dither_pie_amd import backend
    n, h, w = N_TABLE, 2, 3
    assert 65535 % PERIOD != 0
    spec, P = _table_palette(orc, 21)
    base = _base(orc, h, w, 900)
    refs = pattern_ref.pattern_frames(orc, base, *spec, matrix, 128, y0=y0, x0=x0)
    assert len(np.unique(refs.reshape(PERIOD, -1), axis=0)) > PERIOD // 2         # the frames differ: an offset error shows
    got = backend.pattern(torch.from_numpy(_tile(base, n)).cuda(), P, matrix, 128, y0=y0, x0=x0).cpu().numpy()
    _assert_every_frame(got, refs, f"pattern {matrix} {n} x {h}x{w}")


def test_dot_diffusion_in_groups_of_65535_frames(orc):
    import torch
    from dither_pie_amd import backend
    n, h, w = N_TABLE, 2, 3
    assert 65535 % PERIOD != 0
    spec, P = _table_palette(orc, 22)
    base = _base(orc, h, w, 1000)
    refs = dotdiff_ref.dotdiff_frames(orc, base, *spec, dotdiff_ref.KNUTH, 256)
    assert len(np.unique(refs.reshape(PERIOD, -1), axis=0)) > PERIOD // 2
    got = backend.dotdiff(torch.from_numpy(_tile(base, n)).cuda(), P, dotdiff_ref.KNUTH, 256).cpu().numpy()
    _assert_every_frame(got, refs, f"dot diffusion {n} x {h}x{w}")


def test_cells_and_their_sets_plane_in_groups_of_65535_frames(orc):
    """(5, 6) frames in 4 x 4 cells: four cells per frame, three of them partial.  The sets plane is a region of a guarded arena,
    exactly 2 bytes per cell long and 2-byte aligned, no better."""
    import torch
    from dither_pie_amd import backend
    n, h, w = N_TABLE, 5, 6
    assert 65535 % PERIOD != 0
    spec, P = _table_palette(orc, 23)
    base = _base(orc, h, w, 1100)
    refs, ref_sets = cells_ref.cells_frames(base, *spec, 4, 4, 2, 0, [0xFFFF], 4, 64)
    assert ref_sets.shape == (PERIOD, 2, 2) and len(np.unique(ref_sets.reshape(PERIOD, -1), axis=0)) > PERIOD // 2
    g = ar.MIN_GUARD
    A = ar.Arena(ar.capacity_for([(2 * 4 * n, g)]), "cuda", 41)
    A.carve("sets", 2 * 4 * n, 2, g)
    A.fill("sets", ar.noise(42))
    assert A.ptr("sets") % 4 == 2
    sets = A.view("sets").view(torch.uint16)
    assert sets.data_ptr() == A.ptr("sets") and sets.numel() == 4 * n
    out, got_sets = backend.cells(torch.from_numpy(_tile(base, n)).cuda(), P, (4, 4), 2, 4, 64, sets=sets)
    torch.cuda.synchronize()
    assert got_sets.data_ptr() == A.ptr("sets") and tuple(got_sets.shape) == (n, 2, 2)
    A.check()
    _assert_every_frame(out.cpu().numpy(), refs, f"cells {n} x {h}x{w}")
    _assert_every_frame(A.get("sets", np.uint16).reshape(n, 2, 2), ref_sets, f"cells, the sets plane {n} x 2x2")
    del sets, got_sets, A


@pytest.mark.parametrize("mode", [MODE_NEAREST, MODE_MATRIX], ids=["nearest", "bayer4"])
@pytest.mark.parametrize("h,w,residue", [(2, 3, 2), (2, 4, 0)], ids=["bytes", "dwords"])
def test_oklab_ordered_in_groups_of_65535_frames(orc, h, w, residue, mode):
    """Frames of 18 bytes take the byte path, frames of 24 bytes the 12-byte dword path of several frames."""
    import torch
    from dither_pie_amd import backend
    n = N_TABLE
    assert 65535 % PERIOD != 0 and (3 * h * w) % 4 == residue
    pal, outc, _ = orc.prepare_palette(orc.palr(16, 24), False)
    P = backend.Palette(pal, outc, metric="oklab")
    base = _base(orc, h, w, 1200)
    m = orc.bayer_matrix("4x4")
    assert m.shape == (4, 4)
    dev = torch.from_numpy(_tile(base, n)).cuda()
    assert dev.data_ptr() % 4 == 0
    if mode == MODE_NEAREST:
        refs = metric_ref.ordered_u8(base, pal, outc)
        got = backend.ordered(dev, P, MODE_NEAREST)
    else:
        refs = metric_ref.ordered_u8(base, pal, outc, m, 5, 3)
        got = backend.ordered(dev, P, MODE_MATRIX, thr=backend.Thresholds.from_matrix(m), y0=5, x0=3)
        assert not np.array_equal(refs, metric_ref.ordered_u8(base, pal, outc))
    assert got.data_ptr() % 4 == 0
    _assert_every_frame(got.cpu().numpy(), refs, f"oklab ordered, mode {mode}, {n} x {h}x{w}")


def test_integer_diffusion_and_its_workspace_in_groups_of_65535_frames(orc):
    """dp_idiff_u8 itself, as tests/test_gpu_idiff_memory.py calls it: input, output and workspace are regions of one guarded
    arena; the workspace has exactly dp_idiff_workspace_bytes(n, 2, 3) = 32 n 3 bytes, 16-byte aligned and no better, and holds
    noise."""
    import torch
    from dither_pie_amd import _lib, backend
    L = _lib.load()
    n, h, w = N_TABLE, 2, 3
    assert 65535 % PERIOD != 0
    spec, P = _table_palette(orc, 25)
    taps, divisor = idiff_ref.KERNELS["floyd_steinberg"]
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))
    base = _base(orc, h, w, 1300)
    refs = idiff_ref.idiff_frames(orc, base, *spec, taps, divisor, 256)
    assert len(np.unique(refs.reshape(PERIOD, -1), axis=0)) > PERIOD // 2
    frames = _tile(base, n)
    need = L.dp_idiff_workspace_bytes(n, h, w)
    assert need == 32 * n * 3
    g = ar.guard_bytes(frames.nbytes)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g), (need, g)]), "cuda", 51)
    A.carve("in", frames.nbytes, 1, g)
    A.put("in", frames)
    A.carve("out", frames.nbytes, 7, g)
    A.fill("out", ar.noise(52))
    A.carve("ws", need, 0, g)
    A.fill("ws", ar.noise(53))
    assert A.ptr("in") % 2 == 1 and A.ptr("out") % 2 == 1 and A.ptr("ws") % 32 == 16
    rc = L.dp_idiff_u8(A.ptr("in"), A.ptr("out"), n, h, w, P._h, dx.ctypes.data, dy.ctypes.data, wt.ctypes.data, len(taps), divisor, 256,
                       A.ptr("ws"), need, backend._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.dp_last_error())
    A.check()
    A.unchanged("in")
    _assert_every_frame(A.get("out").reshape(n, h, w, 3), refs, f"integer diffusion {n} x {h}x{w}")
    del A


@pytest.mark.parametrize("mode", [MODE_NEAREST, MODE_MATRIX], ids=["nearest", "bayer4"])
def test_rgb_ordered_more_than_65535_frames(orc, mode):
    import torch
    from dither_pie_amd import backend
    n, h, w = N_TABLE, 2, 3
    spec, P = _table_palette(orc, 26)
    base = _base(orc, h, w, 1400)
    m = orc.bayer_matrix("4x4")
    dev = torch.from_numpy(_tile(base, n)).cuda()
    if mode == MODE_NEAREST:
        refs = np.stack([orc.ordered_u8(f, *spec, "none") for f in base])
        got = backend.ordered(dev, P, MODE_NEAREST)
    else:
        refs = np.stack([orc.ordered_u8(f, *spec, "matrix", thr=m) for f in base])
        got = backend.ordered(dev, P, MODE_MATRIX, thr=backend.Thresholds.from_matrix(m))
        assert not np.array_equal(refs, np.stack([orc.ordered_u8(f, *spec, "none") for f in base]))
    _assert_every_frame(got.cpu().numpy(), refs, f"rgb ordered, mode {mode}, {n} x {h}x{w}")
