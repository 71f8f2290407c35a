"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_pattern.h on the guarded arena
(tests/arena.py), as tests/test_gpu_scene_memory.py is for the scene header: the frames the library sees lie inside one
arena, have exactly their size and sit at odd addresses; whatever the output held before -- zeros, 0xFF, noise -- the
pixels are those of tests/pattern_ref.py; guards of >= 1 MiB stay intact; inputs are unchanged; a refused call launches
nothing and leaves every buffer as it was.  dp_pattern_prepare takes no buffer of the caller's: it is run with the arena
live (its table and scratch are the library's own allocations) and must leave guards and regions alone, and the call that
follows must give the pixels of the lazy path.  tests/test_pattern_cpu.py checks COVERAGE against the header.
No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import pattern_ref as pr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_pattern_u8": ["test_pattern_on_the_arena"],
    "dp_pattern_prepare": ["test_pattern_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(91))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, frames, h, w, matrix, strength256, colours, gamma, residues of in / out (odd, and different), prepare first
@pytest.mark.parametrize("case, n, h, w, m, s, k, gamma, r_in, r_out, prepare", [
    (0, 3, 17, 33, 4, 128, 16, False, 1, 7, False),
    (1, 2, 67, 129, 8, 256, 256, False, 3, 5, True),
    (2, 1, 1, 7, 2, 77, 5, True, 15, 9, True),
    (3, 2, 3, 5, 8, 200, 2, False, 5, 11, False),
])
def test_pattern_on_the_arena(gpu, orc, case, n, h, w, m, s, k, gamma, r_in, r_out, prepare):
    import torch
    from dither_pie_amd.dithering_lib import prepare_palette
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(50 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    pal_f32, outc, lut = prepare_palette([tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], gamma)
    want = pr.pattern_frames(orc, frames, pal_f32, outc, lut, m, s, y0=case, x0=2 * case + 1)
    P = be.Palette(pal_f32, outc, lut)
    specs = [(frames.nbytes, g), (frames.nbytes, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 70 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes at an odd address
    A.put("in", frames)
    A.carve("out", frames.nbytes, r_out, g)
    assert A.ptr("in") % 2 == 1 and A.ptr("out") % 2 == 1 and A.ptr("in") % 16 != A.ptr("out") % 16
    st = be._stream()
    if prepare:
        A.fill("out", FILLS[0])
        assert L.dp_pattern_prepare(P._h) == DP_OK, L.dp_last_error()
        assert L.dp_pattern_prepare(P._h) == DP_OK                      # idempotent
        torch.cuda.synchronize()
        A.check()
        A.unchanged("in")
        A.unchanged("out")
    assert L.dp_pattern_table_bytes(P._h) == (1 << 24) + 3 * 1024
    for i, fill in enumerate(FILLS):
        A.reseed(800 + 10 * case + i)
        A.fill("out", fill)
        rc = L.dp_pattern_u8(A.ptr("in"), A.ptr("out"), n, h, w, case, 2 * case + 1, P._h, m, s, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("out").reshape(n, h, w, 3), want), (case, fill)
        A.check()
        A.unchanged("in")

    # refusals launch nothing: every buffer keeps what it holds
    A.put("out", A.get("out").copy())
    for kw in (dict(i=None), dict(o=None), dict(h=0), dict(w=-1), dict(y0=-1), dict(x0=-3), dict(m=3), dict(m=16), dict(s=-1), dict(s=257),
               dict(pal=None), dict(n=-1)):
        v = dict(i=A.ptr("in"), o=A.ptr("out"), n=n, h=h, w=w, y0=0, x0=0, pal=P._h, m=m, s=s)
        v.update(kw)
        rc = L.dp_pattern_u8(v["i"], v["o"], v["n"], v["h"], v["w"], v["y0"], v["x0"], v["pal"], v["m"], v["s"], st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_pattern_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_pattern_u8(A.ptr("in"), A.ptr("out"), 0, h, w, 0, 0, P._h, m, s, st) == DP_OK       # n_frames = 0: a no-op
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("out")
    A.check()
    del A


def test_unsupported_palettes_are_refused_and_launch_nothing(gpu):
    """More than 256 colours, and a palette value outside [0, 255] (a real dp_palette is needed to hold one)."""
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
    big = rs.randint(0, 256, (300, 3)).astype(np.float32)
    wide = np.array([[0, 0, 0], [255.5, 10, 10], [20, 20, 20]], np.float32)
    low = np.array([[0, 0, 0], [10, -0.25, 10]], np.float32)
    for pal, word in ((big, b"256"), (wide, b"[0, 255]"), (low, b"[0, 255]")):
        P = be.Palette(pal, np.clip(pal, 0, 255).astype(np.uint8), None)
        rc = L.dp_pattern_u8(A.ptr("in"), A.ptr("out"), 2, 5, 9, 0, 0, P._h, 4, 128, be._stream())
        torch.cuda.synchronize()
        assert rc == DP_EUNSUPPORTED and b"dp_pattern_u8" in L.dp_last_error() and word in L.dp_last_error(), (rc, L.dp_last_error())
        rc = L.dp_pattern_prepare(P._h)
        assert rc == DP_EUNSUPPORTED and b"dp_pattern_prepare" in L.dp_last_error(), (rc, L.dp_last_error())
        assert L.dp_pattern_table_bytes(P._h) == 0
        with pytest.raises((ValueError, be.DitherPieError)):
            be.pattern(torch.from_numpy(frames).cuda(), P, 4, 128)
    A.unchanged("in")
    A.unchanged("out")
    A.check()
    del A
