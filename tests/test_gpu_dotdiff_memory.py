"""GPU tier: memory discipline of the device entry point of include/ditherpie_hip_dotdiff.h on the guarded arena
(tests/arena.py), as tests/test_gpu_pattern_memory.py is for the pattern header: the frames the library sees lie inside one
arena, have exactly their size and sit at odd addresses; whatever the output held before -- zeros, 0xFF, noise -- the
pixels are those of tests/dotdiff_ref.py; guards of >= 1 MiB stay intact; the input is unchanged; a refused call launches
nothing and leaves every buffer as it was.  One case has three tiles each way, so that the halo reads of the edge tiles stop
at the frame's first and last byte, and two frames, so that the halo of one frame's tiles stops at its neighbour.
tests/test_dotdiff_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import dotdiff_ref as dr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_dotdiff_u8": ["test_dotdiff_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(93))
T = 64   # backend.DOTDIFF_TILE


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    assert backend.DOTDIFF_TILE == T
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _matrix(m, seed):
    """A class matrix of size m whose reach the kernel takes: drawn until one fits (the first draw nearly always does)."""
    rs = np.random.RandomState(seed)
    while True:
        M = rs.permutation(m * m).reshape(m, m)
        if dr.reach(M) <= dr.MAX_REACH:
            return M


# case, frames, h, w, matrix size (0: the default matrix), strength256, colours, gamma, residues of in / out, prepare first
@pytest.mark.parametrize("case, n, h, w, m, s, k, gamma, r_in, r_out, prepare", [
    (0, 3, 17, 33, 0, 256, 16, False, 1, 7, False),
    (1, 2, 2 * T + 19, 3 * T + 5, 16, 256, 256, False, 3, 5, True),
    (2, 1, 1, 7, 2, 77, 5, True, 15, 9, True),
    (3, 2, 3, 5, 4, 200, 2, False, 5, 11, False),
])
def test_dotdiff_on_the_arena(gpu, orc, case, n, h, w, m, s, k, gamma, r_in, r_out, prepare):
    import torch
    from dither_pie_amd.dithering_lib import prepare_palette
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(60 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    pal_f32, outc, lut = prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], gamma)
    M = np.ascontiguousarray(dr.KNUTH if m == 0 else _matrix(m, 70 + case), np.uint8)
    m = M.shape[0]
    want = dr.dotdiff_frames(orc, frames, pal_f32, outc, lut, M, s)
    P = be.Palette(pal_f32, outc, lut)
    specs = [(frames.nbytes, g), (frames.nbytes, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 80 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes at an odd address
    A.put("in", frames)
    A.carve("out", frames.nbytes, r_out, g)
    assert A.ptr("in") % 2 == 1 and A.ptr("out") % 2 == 1 and A.ptr("in") % 16 != A.ptr("out") % 16
    st = be._stream()
    if prepare:                                                         # the table built ahead by the pattern header's call
        assert L.dp_pattern_prepare(P._h) == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
    for i, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + i)
        A.fill("out", fill)
        rc = L.dp_dotdiff_u8(A.ptr("in"), A.ptr("out"), n, h, w, P._h, M.ctypes.data, m, s, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("out").reshape(n, h, w, 3), want), (case, fill)
        A.check()
        A.unchanged("in")
    assert L.dp_pattern_table_bytes(P._h) == (1 << 24) + 3 * 1024

    # refusals launch nothing: every buffer keeps what it holds
    A.put("out", A.get("out").copy())
    twice = M.copy()
    twice.reshape(-1)[1] = twice.reshape(-1)[0]                         # a repeated class
    for kw, code in ((dict(i=None), DP_EINVAL), (dict(o=None), DP_EINVAL), (dict(h=0), DP_EINVAL), (dict(w=-1), DP_EINVAL),
                     (dict(m=3), DP_EINVAL), (dict(m=32), DP_EINVAL), (dict(s=-1), DP_EINVAL), (dict(s=257), DP_EINVAL),
                     (dict(pal=None), DP_EINVAL), (dict(n=-1), DP_EINVAL), (dict(c=None), DP_EINVAL),
                     (dict(c=twice.ctypes.data), DP_EINVAL), (dict(o=A.ptr("in")), DP_EINVAL)):
        v = dict(i=A.ptr("in"), o=A.ptr("out"), n=n, h=h, w=w, pal=P._h, c=M.ctypes.data, m=m, s=s)
        v.update(kw)
        rc = L.dp_dotdiff_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["pal"], v["c"], v["m"], v["s"], st)
        torch.cuda.synchronize()
        assert rc == code and b"dp_dotdiff_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_dotdiff_u8(A.ptr("in"), A.ptr("out"), 0, h, w, P._h, M.ctypes.data, m, s, st) == DP_OK   # n_frames = 0: a no-op
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("out")
    A.check()
    del A


def test_unsupported_palettes_and_matrices_are_refused_and_launch_nothing(gpu):
    """More than 256 colours, a palette value outside [0, 255] (a real dp_palette is needed to hold one), a reach of 17."""
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    frames = np.random.RandomState(1).randint(0, 256, (2, 5, 9, 3)).astype(np.uint8)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g)]), "cuda", 3)
    A.carve("in", frames.nbytes, 1, g)
    A.put("in", frames)
    A.carve("out", frames.nbytes, 3, g)
    A.fill("out", FILLS[2])
    rs = np.random.RandomState(2)
    M = np.ascontiguousarray(dr.KNUTH, np.uint8)
    big = rs.randint(0, 256, (300, 3)).astype(np.float32)
    wide = np.array([[0, 0, 0], [255.5, 10, 10], [20, 20, 20]], np.float32)
    low = np.array([[0, 0, 0], [10, -0.25, 10]], np.float32)
    for pal, word in ((big, b"256"), (wide, b"[0, 255]"), (low, b"[0, 255]")):
        P = be.Palette(pal, np.clip(pal, 0, 255).astype(np.uint8), None)
        rc = L.dp_dotdiff_u8(A.ptr("in"), A.ptr("out"), 2, 5, 9, P._h, M.ctypes.data, 8, 256, be._stream())
        torch.cuda.synchronize()
        assert rc == DP_EUNSUPPORTED and b"dp_dotdiff_u8" in L.dp_last_error() and word in L.dp_last_error(), (rc, L.dp_last_error())
        with pytest.raises((ValueError, be.DitherPieError)):
            be.dotdiff(torch.from_numpy(frames).cuda(), P, M, 256)
    ok = rs.randint(0, 256, (4, 3)).astype(np.float32)
    P = be.Palette(ok, ok.astype(np.uint8), None)
    rs17 = np.random.RandomState(2032)
    far = next(c for c in (np.ascontiguousarray(rs17.permutation(64).reshape(8, 8), np.uint8) for _ in range(2000)) if dr.reach(c) == 17)
    rc = L.dp_dotdiff_u8(A.ptr("in"), A.ptr("out"), 2, 5, 9, P._h, far.ctypes.data, 8, 256, be._stream())
    torch.cuda.synchronize()
    assert rc == DP_EUNSUPPORTED and b"dp_dotdiff_u8" in L.dp_last_error() and b"reach 17" in L.dp_last_error(), (rc, L.dp_last_error())
    A.unchanged("in")
    A.unchanged("out")
    A.check()
    del A
