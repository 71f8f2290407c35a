"""GPU tier: memory discipline of the device entry point of include/ditherpie_hip_cells.h on the guarded arena
(tests/arena.py), as tests/test_gpu_dotdiff_memory.py is for the dot-diffusion header: the frames the library sees lie inside
one arena, have exactly their size and sit at odd addresses, the masks at an even one that is no better aligned; whatever
the outputs held before -- zeros, 0xFF, noise -- pixels and masks are those of tests/cells_ref.py; guards of >= 1 MiB stay
intact; the input is unchanged out of place; one case works in place; a refused call launches nothing and leaves every
buffer as it was.  Every shape cuts its cells at the right and the bottom edge, where a lane without a pixel must neither
read nor write.  tests/test_cells_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import cells_ref as cr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_cells_u8": ["test_cells_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(94))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, frames, h, w, cw, ch, colours, fixed, groups, m, spread, palette size, gamma, residues of in / out / sets, in place
@pytest.mark.parametrize("case, n, h, w, cw, ch, k, fixed, groups, m, spread, K, gamma, r_in, r_out, r_sets, inplace", [
    (0, 1, 17, 33, 8, 8, 2, 0, (0xFFFF,), 4, 64, 16, False, 1, 7, 2, False),
    (1, 3, 1, 7, 4, 4, 1, 0b10, (0b00111, 0b11100), 2, 255, 5, True, 15, 9, 6, False),
    (2, 2, 35, 19, 16, 16, 4, 0, (0x00FF, 0x7F01), 8, 128, 15, False, 3, 5, 10, False),
    (3, 2, 17, 33, 8, 8, 3, 0b1, (0xFFFF,), 4, 64, 16, True, 5, 5, 14, True),
])
def test_cells_on_the_arena(gpu, case, n, h, w, cw, ch, k, fixed, groups, m, spread, K, gamma, r_in, r_out, r_sets, inplace):
    import torch
    from dither_pie_amd.dithering_lib import prepare_palette
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(160 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    pal_f32, outc, lut = prepare_palette([tuple(c) for c in rs.randint(0, 256, (K, 3)).tolist()], gamma)
    want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, cw, ch, k, fixed, list(groups), m, spread)
    grp = np.array(groups, np.uint16)
    P = be.Palette(pal_f32, outc, lut)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g), (want_sets.nbytes, g)]), "cuda", 180 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes at an odd address
    A.put("in", frames)
    if not inplace:
        A.carve("out", frames.nbytes, r_out, g)
    A.carve("sets", want_sets.nbytes, r_sets, g)                        # exactly 2 bytes per cell at an even, not a 4-byte address
    o = "in" if inplace else "out"
    assert A.ptr("in") % 2 == 1 and A.ptr(o) % 2 == 1 and A.ptr("sets") % 4 == 2
    st = be._stream()

    def call(**kw):
        v = dict(i=A.ptr("in"), o=A.ptr(o), s=A.ptr("sets"), n=n, h=h, w=w, pal=P._h, cw=cw, ch=ch, k=k, fixed=fixed, g=grp.ctypes.data,
                 ng=len(grp), m=m, spread=spread)
        v.update(kw)
        rc = L.dp_cells_u8(v["i"], v["o"], v["s"], v["n"], v["h"], v["w"], v["pal"], v["cw"], v["ch"], v["k"], v["fixed"], v["g"], v["ng"],
                           v["m"], v["spread"], st)
        torch.cuda.synchronize()
        return rc

    for i, fill in enumerate(FILLS):
        A.reseed(1900 + 10 * case + i)
        if inplace:
            A.put("in", frames)
        else:
            A.fill("out", fill)
        A.fill("sets", fill)
        rc = call()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("sets", np.uint16).reshape(want_sets.shape), want_sets), (case, fill)
        assert np.array_equal(A.get(o).reshape(n, h, w, 3), want), (case, fill)
        A.check()
        if not inplace:
            A.unchanged("in")
    # without the masks: the same pixels, the masks' region untouched
    A.put("sets", A.get("sets").copy())
    if inplace:
        A.put("in", frames)
    else:
        A.fill("out", FILLS[2])
    assert call(s=None) == DP_OK, L.dp_last_error()
    assert np.array_equal(A.get(o).reshape(n, h, w, 3), want)
    A.unchanged("sets")
    A.check()

    # refusals launch nothing: every buffer keeps what it holds
    A.put(o, A.get(o).copy())
    empty, small = np.array([0], np.uint16), np.array([0b11], np.uint16)
    beyond = np.array([1 << K if K < 16 else 0], np.uint16)              # a bit at K (K = 16: no such mask, an empty group instead)
    for kw, code in ((dict(i=None), DP_EINVAL), (dict(o=None), DP_EINVAL), (dict(pal=None), DP_EINVAL), (dict(g=None), DP_EINVAL),
                     (dict(n=-1), DP_EINVAL), (dict(h=0), DP_EINVAL), (dict(w=-1), DP_EINVAL), (dict(h=1 << 16, w=1 << 16), DP_EINVAL),
                     (dict(cw=2), DP_EINVAL), (dict(cw=32), DP_EINVAL), (dict(ch=12), DP_EINVAL), (dict(m=3), DP_EINVAL), (dict(m=16), DP_EINVAL),
                     (dict(k=0), DP_EINVAL), (dict(k=5), DP_EINVAL), (dict(spread=-1), DP_EINVAL), (dict(spread=256), DP_EINVAL),
                     (dict(ng=0), DP_EINVAL), (dict(ng=5), DP_EINVAL), (dict(fixed=1 << K), DP_EINVAL),
                     (dict(g=beyond.ctypes.data, ng=1), DP_EINVAL), (dict(g=empty.ctypes.data, ng=1), DP_EINVAL),
                     (dict(g=small.ctypes.data, ng=1, k=3, fixed=0), DP_EINVAL), (dict(g=small.ctypes.data, ng=1, k=2, fixed=1), DP_EINVAL),
                     (dict(s=A.ptr("sets") + 1), DP_EINVAL)):
        rc = call(**kw)
        assert rc == code and b"dp_cells_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert call(n=0) == DP_OK                                            # n_frames = 0: a no-op
    A.unchanged("in")
    if not inplace:
        A.unchanged("out")
    A.unchanged("sets")
    A.check()
    del A


def test_unsupported_palettes_are_refused_and_launch_nothing(gpu):
    """More than 16 colours, a palette value outside [0, 255] (a real dp_palette is needed to hold one)."""
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    frames = np.random.RandomState(1).randint(0, 256, (2, 5, 9, 3)).astype(np.uint8)
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (frames.nbytes, g), (8, g)]), "cuda", 3)
    A.carve("in", frames.nbytes, 1, g)
    A.put("in", frames)
    A.carve("out", frames.nbytes, 3, g)
    A.fill("out", FILLS[2])
    A.carve("sets", 8, 2, g)
    A.fill("sets", FILLS[2])
    rs = np.random.RandomState(2)
    big = rs.randint(0, 256, (17, 3)).astype(np.float32)
    wide = np.array([[0, 0, 0], [255.5, 10, 10], [20, 20, 20]], np.float32)
    low = np.array([[0, 0, 0], [10, -0.25, 10]], np.float32)
    for pal, word in ((big, b"16"), (wide, b"[0, 255]"), (low, b"[0, 255]")):
        P = be.Palette(pal, np.clip(pal, 0, 255).astype(np.uint8), None)
        grp = np.array([0b11], np.uint16)
        rc = L.dp_cells_u8(A.ptr("in"), A.ptr("out"), A.ptr("sets"), 2, 5, 9, P._h, 8, 8, 2, 0, grp.ctypes.data, 1, 4, 64, be._stream())
        torch.cuda.synchronize()
        assert rc == DP_EUNSUPPORTED and b"dp_cells_u8" in L.dp_last_error() and word in L.dp_last_error(), (rc, L.dp_last_error())
        with pytest.raises((ValueError, be.DitherPieError)):
            be.cells(torch.from_numpy(frames).cuda(), P, (8, 8), 2, 4, 64, groups=[0b11])
    A.unchanged("in")
    A.unchanged("out")
    A.unchanged("sets")
    A.check()
    del A
