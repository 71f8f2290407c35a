"""GPU tier: memory discipline of the device entry point of include/ditherpie_hip_idiff.h on the guarded arena (tests/arena.py),
as tests/test_gpu_dotdiff_memory.py is for the dot-diffusion header: the frames the library sees lie inside one arena, have
exactly their size and sit at odd addresses; the workspace has exactly dp_idiff_workspace_bytes bytes, 16-byte aligned and no
better, and holds noise; whatever the output held before -- zeros, 0xFF, noise -- the pixels are those of tests/idiff_ref.py;
guards of >= 1 MiB stay intact; the input is unchanged; a refused call launches nothing and leaves every buffer as it was.
One case is (2, 130, 70): band boundaries, the wrap of the 64-column ring and the frame boundary all sit against guards (the
unaligned dword loads and stores of the first and the last period of a frame must stop at its first and last byte).
tests/test_idiff_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import idiff_ref as ir

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_idiff_u8": ["test_idiff_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED, DP_EWORKSPACE = 0, 1, 2, 5
FILLS = ("zeros", "ones", ar.noise(93))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _call(L, v, st):
    return L.dp_idiff_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["pal"], v["dx"], v["dy"], v["wt"], v["nt"], v["d"], v["s"], v["ws"], v["wsb"], st)


# case, frames, h, w, variant, strength256, colours, gamma, metric, residues of in / out, prepare first
@pytest.mark.parametrize("case, n, h, w, name, s, k, gamma, metric, r_in, r_out, prepare", [
    (0, 3, 17, 33, "floyd_steinberg", 256, 16, False, "rgb", 1, 7, False),
    (1, 2, 130, 70, "jjn", 256, 256, False, "rgb", 3, 5, True),
    (2, 1, 1, 7, "atkinson", 77, 5, True, "rgb", 15, 9, True),
    (3, 2, 3, 5, "sierra_lite", 200, 2, False, "oklab", 5, 11, False),
    (4, 1, 65, 16, "burkes", 256, 16, False, "oklab", 13, 3, True),
])
def test_idiff_on_the_arena(gpu, orc, case, n, h, w, name, s, k, gamma, metric, r_in, r_out, prepare):
    import torch
    import metric_ref as mr
    from dither_pie_amd.dithering_lib import prepare_palette
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(60 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    pal_f32, outc, lut = prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], gamma)
    taps, divisor = ir.KERNELS[name]
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))   # exactly n_taps each
    want = ir.idiff_frames(orc if metric == "rgb" else mr.NearestAdapter(metric), frames, pal_f32, outc, lut, taps, divisor, s)
    P = be.Palette(pal_f32, outc, lut) if metric == "rgb" else be.Palette(pal_f32, outc, metric=metric)
    need = L.dp_idiff_workspace_bytes(n, h, w)
    assert need == 32 * n * w
    specs = [(frames.nbytes, g), (frames.nbytes, g), (need, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 80 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes at an odd address
    A.put("in", frames)
    A.carve("out", frames.nbytes, r_out, g)
    A.carve("ws", need, 0, g)                                           # exactly the bytes asked for, 16-byte aligned and no better
    assert A.ptr("in") % 2 == 1 and A.ptr("out") % 2 == 1 and A.ptr("in") % 16 != A.ptr("out") % 16 and A.ptr("ws") % 32 == 16
    st = be._stream()
    if prepare:                                                         # the tables built ahead by their own headers' calls
        if metric != "rgb":
            P.metric_prepare()
        assert L.dp_pattern_prepare(P._h) == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
    ok = dict(i=A.ptr("in"), o=A.ptr("out"), n=n, h=h, w=w, pal=P._h, dx=dx.ctypes.data, dy=dy.ctypes.data, wt=wt.ctypes.data, nt=len(taps),
              d=divisor, s=s, ws=A.ptr("ws"), wsb=need)
    for i, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + i)
        A.fill("out", fill)
        A.fill("ws", FILLS[(i + 1) % 3])                                # whatever the workspace held
        rc = _call(L, ok, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        got = A.get("out").reshape(n, h, w, 3)
        bad = np.argwhere((got != want).any(axis=-1))
        assert not len(bad), (case, fill, len(bad), bad[:4].tolist())
        A.check()
        A.unchanged("in")

    # refusals launch nothing: every buffer keeps what it holds
    A.put("out", A.get("out").copy())
    A.put("ws", A.get("ws").copy())
    twice = dx.copy(), dy.copy()
    if len(taps) > 1:
        twice[0][1], twice[1][1] = twice[0][0], twice[1][0]             # a (dx, dy) given twice
    else:
        twice[0][0] = 3                                                 # (one tap: outside the window instead)
    neg = wt.copy()
    neg[0] = -1
    for kw, code in ((dict(i=None), DP_EINVAL), (dict(o=None), DP_EINVAL), (dict(ws=None), DP_EINVAL), (dict(h=0), DP_EINVAL),
                     (dict(w=-1), DP_EINVAL), (dict(nt=0), DP_EINVAL), (dict(nt=13), DP_EINVAL), (dict(s=-1), DP_EINVAL), (dict(s=257), DP_EINVAL),
                     (dict(d=0), DP_EINVAL), (dict(d=sum(t[2] for t in taps) - 1), DP_EINVAL), (dict(pal=None), DP_EINVAL), (dict(n=-1), DP_EINVAL),
                     (dict(dx=None), DP_EINVAL), (dict(dy=None), DP_EINVAL), (dict(wt=None), DP_EINVAL), (dict(wt=neg.ctypes.data), DP_EINVAL),
                     (dict(dx=twice[0].ctypes.data, dy=twice[1].ctypes.data), DP_EINVAL), (dict(o=A.ptr("in")), DP_EINVAL),
                     (dict(ws=A.ptr("ws") + 8, wsb=need - 8), DP_EINVAL), (dict(ws=A.ptr("ws") + 1), DP_EINVAL),
                     (dict(wsb=need - 1), DP_EWORKSPACE), (dict(wsb=0), DP_EWORKSPACE)):
        rc = _call(L, dict(ok, **kw), st)
        torch.cuda.synchronize()
        assert rc == code and b"dp_idiff_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert _call(L, dict(ok, n=0), st) == DP_OK                         # n_frames = 0: a no-op
    assert _call(L, dict(ok, n=0, i=None, o=None, ws=None, wsb=0), st) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("out")
    A.unchanged("ws")
    A.check()
    del A


def test_unsupported_palettes_are_refused_and_launch_nothing(gpu):
    """More than 256 colours, a palette value outside [0, 255] (a real dp_palette is needed to hold one)."""
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    frames = np.random.RandomState(1).randint(0, 256, (2, 5, 9, 3)).astype(np.uint8)
    need = L.dp_idiff_workspace_bytes(2, 5, 9)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g), (need, g)]), "cuda", 3)
    A.carve("in", frames.nbytes, 1, g)
    A.put("in", frames)
    A.carve("out", frames.nbytes, 3, g)
    A.fill("out", FILLS[2])
    A.carve("ws", need, 0, g)
    A.fill("ws", FILLS[1])
    rs = np.random.RandomState(2)
    taps, divisor = ir.KERNELS["floyd_steinberg"]
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))
    big = rs.randint(0, 256, (300, 3)).astype(np.float32)
    wide = np.array([[0, 0, 0], [255.5, 10, 10], [20, 20, 20]], np.float32)
    low = np.array([[0, 0, 0], [10, -0.25, 10]], np.float32)
    for pal, word in ((big, b"256"), (wide, b"[0, 255]"), (low, b"[0, 255]")):
        P = be.Palette(pal, np.clip(pal, 0, 255).astype(np.uint8), None)
        rc = L.dp_idiff_u8(A.ptr("in"), A.ptr("out"), 2, 5, 9, P._h, dx.ctypes.data, dy.ctypes.data, wt.ctypes.data, 4, divisor, 256, A.ptr("ws"), need,
                           be._stream())
        torch.cuda.synchronize()
        assert rc == DP_EUNSUPPORTED and b"dp_idiff_u8" in L.dp_last_error() and word in L.dp_last_error(), (rc, L.dp_last_error())
        with pytest.raises((ValueError, be.DitherPieError)):
            be.idiff(torch.from_numpy(frames).cuda(), P, taps, divisor, 256)
    A.unchanged("in")
    A.unchanged("out")
    A.unchanged("ws")
    A.check()
    del A
