"""CPU tier of the colour-cube tests: the helper (tests/cube_ref.py) and the identities the GPU tier
(tests/test_gpu_colour_cube.py) builds its expectations on, each shown with the oracle alone."""
import numpy as np
import pytest

import cube_ref as cr

# the palettes whose error-diffusion candidate lists the GPU tier walks at every integer point
ED_PALETTES = ("two", "palr16", "palr256", "clustered200", "mc64", "dup256")
SLICE = 256   # a 256 x 256 slice of a cube: pixels 0 .. 65535 of the cube's own order


def _slices():
    """256 x 256 slices of both cubes: the identity cube's first 65536 pixels are the one plane r = 0, so the identity slice
    takes every 256th pixel with b moved along (row y, column x: colour (y, x, y)), the scattered one the cube's first pixels"""
    p = np.arange(SLICE * SLICE, dtype=np.int64)
    ident = cr.colours_of(p * 256 + (p >> 8)).reshape(SLICE, SLICE, 3)
    scat = cr.colours_of((p * cr.M) & (cr.N - 1)).reshape(SLICE, SLICE, 3)
    return {"identity": ident, "scattered": scat}


def test_both_cubes_hold_every_colour_once():
    perm = cr.scatter_index()
    assert cr.M % 2 == 1 and cr.M >> 23 == 1 and cr.M & 0xF
    assert np.array_equal(np.sort(perm), np.arange(cr.N))
    for cube, order in ((cr.identity_cube(), np.arange(cr.N)), (cr.scattered_cube(), perm)):
        assert cube.shape == (cr.SIDE, cr.SIDE, 3) and cube.dtype == np.uint8
        c = cube.reshape(-1, 3).astype(np.int64)
        assert np.array_equal((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2], order)
    # neighbours of the scattered order sit in unrelated cells: no two of a group of four share one
    cells = (perm >> 20 << 8) | ((perm >> 12) & 15) << 4 | ((perm >> 4) & 15)
    g = cells.reshape(-1, 4)
    assert all((g[:, i] != g[:, j]).all() for i in range(4) for j in range(i + 1, 4))
    assert len(np.unique(cells[:64])) == 64


def test_gather_inverts_the_scatter():
    """A colour-only operation run on the scattered cube equals its identity result gathered through the bijection."""
    perm = cr.scatter_index()
    ident, scat = cr.identity_cube(), cr.scattered_cube()
    assert np.array_equal(cr.gather(ident, perm), scat)
    f = lambda a: (a.astype(np.int64) @ np.array([3, 5, 7]) % 251).astype(np.uint8)     # any function of the colour
    assert np.array_equal(cr.gather(f(ident), perm), f(scat))


def test_index_colours_decode():
    for K in (1, 2, 255, 256, 257, 1024):
        oc = cr.index_colours(K)
        assert oc.shape == (K, 3) and oc.dtype == np.uint8
        assert np.array_equal(cr.decode(oc), np.arange(K))
        assert len({tuple(c) for c in oc}) == K


def test_palettes_are_what_their_names_say(orc):
    sizes = {"one": 1, "two": 2, "uniform27": 27, "uniform125": 125, "edges64": 64, "palr16": 16, "palr256": 256, "palr300": 300,
             "palr1024": 1024, "dup256": 256, "clustered200": 200, "mc64": 64, "mc256": 256}
    assert set(sizes) == set(cr.PALETTES)
    for name, K in sizes.items():
        pal = cr.palette(orc, name)
        assert len(pal) == K and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in pal), name
    dup = cr.palette(orc, "dup256")
    assert dup[:128] == dup[128:]
    cl = np.array(cr.palette(orc, "clustered200")[:160])
    assert (cl.max(0) - cl.min(0) <= 5).all()
    # with index colours the second copy of a duplicated entry is told from the first
    idx = cr.decode(cr.oracle_pass(orc, _slices()["scattered"], *cr.prepared(orc, "dup256", False), "S"))
    assert (idx >= 128).any() and (idx < 128).any()


@pytest.mark.parametrize("name", ["palr16", "uniform27"])
def test_float_threshold_pass_equals_second_nearest_pass(orc, name):
    """F = S on an integer palette: 2^-20 lies below every non-zero factor, so both thresholds send exactly the colours
    with d0 > 0 to the second entry."""
    for cube in _slices().values():
        p = cr.prepared(orc, name, False)
        s = cr.oracle_pass(orc, cube, *p, "S")
        assert np.array_equal(cr.oracle_pass(orc, cube, *p, "F"), s)
        assert not np.array_equal(s, cr.oracle_pass(orc, cube, *p, "N"))


def test_k1_and_k2_queries_order_ties_differently(orc):
    """Why pass C is run through the oracle and not derived from N and S: on the plane r = 1 both entries of `two` are
    equidistant, the k=1 query picks one of them and the k=2 query lists the other first.  (Threshold 1 keeps the first
    entry of the k=2 query: the factor d0 / (d0 + d1) never exceeds 1/2.)"""
    p = cr.prepared(orc, "two", False)
    g, b = np.mgrid[0:256, 0:256]
    for r in (0, 1, 2, 3):
        plane = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)
        near = cr.decode(cr.oracle_pass(orc, plane, *p, "N"))
        first = cr.decode(orc.ordered_u8(plane, *p, "matrix", thr=np.array([[1.0]], np.float32)))
        if r == 1:
            assert (near != first).all()
        else:
            assert np.array_equal(near, first)
    # ... so a checkerboard put together from N and S is not the oracle's
    cube = _slices()["identity"]      # row y holds r = y: the plane r = 1 is in it
    n, s, c = (cr.oracle_pass(orc, cube, *p, w) for w in ("N", "S", "C"))
    y, x = np.mgrid[0:SLICE, 0:SLICE]
    derived = np.where(((y + x) % 2 == 0)[..., None], s, n)
    assert not np.array_equal(derived, c)
    assert np.array_equal(derived[cube[..., 0] != 1], c[cube[..., 0] != 1])


def _ed_zero_weights(orc, arr, pal_f32, out_colors, lut_in, serpentine):
    """the oracle's error diffusion with the Floyd-Steinberg offsets and all four weights 0.0"""
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    h, w, _ = arr.shape
    out = np.empty_like(arr)
    dx = np.array([1, -1, 0, 1], np.int32)
    dy = np.array([0, 1, 1, 1], np.int32)
    wq = np.zeros(4, np.float64)
    rc = orc.lib().orc_error_diffusion_u8(orc._p(arr), orc._p(out), h, w, orc._p(pal_f32), pal_f32.shape[0], orc._p(out_colors),
                                          orc._p(lut_in), orc._p(dx), orc._p(dy), orc._p(wq), 4, 1 if serpentine else 0)
    assert rc == 0
    return out


@pytest.mark.parametrize("gamma", cr.GAMMAS)
@pytest.mark.parametrize("name", ED_PALETTES)
def test_zero_weight_diffusion_is_the_nearest_pass(orc, name, gamma):
    """With no error pushed every pixel of an error diffusion is a k=1 query at an integer point: pass N."""
    assert [t[:2] for t in orc.ed_kernel("floyd_steinberg")[0]] == [(1, 0), (-1, 1), (0, 1), (1, 1)]
    p = cr.prepared(orc, name, gamma)
    for what, cube in _slices().items():
        want = cr.oracle_pass(orc, cube, *p, "N")
        for serp in (False, True):
            assert np.array_equal(_ed_zero_weights(orc, cube, *p, serp), want), (what, serp)
