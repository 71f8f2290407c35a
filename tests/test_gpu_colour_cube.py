"""GPU tier: the nearest-colour search of every table kind over ALL 2^24 colours (tests/cube_ref.py).

Every ordered mode, the pattern table, the error-diffusion candidate lists and the k-means cell lists claim that a per-cell
candidate structure returns, for one colour, exactly the entry (or the two entries) scipy's KD-tree returns, tie order
included.  Here that is checked colour by colour: the cube is one 4096 x 4096 frame, the CPU oracle answers one pass over it,
the device's output must be equal byte for byte -- in index colours (out_colors[k] spells k), so entries of equal colour and
ties between them count too.  No tolerance anywhere.

  a. the library that ships: every palette of cube_ref.PALETTES, both use_gamma values, every pass, both cubes;
  b. the experiments library: tables and kernels forced by switches, the instantiation each case ran read from the
     DP_ORDERED_TRACE line, and a final test that the cases cover every pass-1 kernel the launcher names but UNREACHED;
  c. the pattern table at strength 0 = pass N;
  d. error diffusion with all weights 0.0 = pass N, in the three frame shapes that reach its three schedules and with each
     candidate structure pinned by switches (the equivalence itself: tests/test_colour_cube_cpu.py);
  e. the k-means passes (full scan, cell lists, histogram) over the cube against orc.kmeans_step.

A mismatch is a bug of the library for that colour: the failure names the count, the first colours and their cells."""
import collections
import re

import numpy as np
import pytest

import cube_ref as cr
from test_ordered_plan_cpu import KERNELS

pytestmark = pytest.mark.gpu

N = cr.N
_HOST = {}     # the identity cube on the host (what the oracle reads)
_DEV = {}      # device tensors shared by the module: the cubes, the bijection, the oracle's answers
_EXPECT = collections.OrderedDict()   # (palette, gamma, pass) -> the oracle's output over the identity cube, on the device, [2^24, 3] uint8
_EXPECT_KEEP = 6   # ... the last few only (48 MB each): the cases of every part are ordered by palette, so few are computed twice


@pytest.fixture
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    yield backend
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _release_the_cubes():
    """the cubes and the oracle's answers (48 MB each) stay on the device while this module runs, not longer"""
    yield
    for cache in (_EXPECT, _DEV, _HOST, _KM_REF):
        cache.clear()
    import torch
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _dev(what):
    import torch
    if not _DEV:
        p = torch.arange(N, device="cuda", dtype=torch.int64)
        perm = (p * cr.M) & (N - 1)

        def colours(q):
            return torch.stack([q >> 16, (q >> 8) & 255, q & 255], -1).to(torch.uint8).view(cr.SIDE, cr.SIDE, 3)
        _DEV.update(identity=colours(p), scattered=colours(perm), perm=perm)
        # (the device-made cubes are the helper's: the CPU tier pins those)
        host = cr.identity_cube()
        assert torch.equal(_DEV["identity"].cpu(), torch.from_numpy(host))
        assert torch.equal(_DEV["perm"][:4096].cpu(), torch.from_numpy(cr.scatter_index()[:4096]))
        _HOST["identity"] = host
    return _DEV[what]


def _expect(orc, name, gamma, which):
    """the oracle's pass over the identity cube, on the device; the last _EXPECT_KEEP answers are kept"""
    import torch
    key = (name, gamma, which)
    if key not in _EXPECT:
        _dev("identity")
        _EXPECT[key] = torch.from_numpy(cr.expected(orc, name, gamma, which, _HOST["identity"])).cuda().view(N, 3)
        while len(_EXPECT) > _EXPECT_KEEP:
            _EXPECT.popitem(last=False)
    _EXPECT.move_to_end(key)
    return _EXPECT[key]


def _same(got, want, order, what, coded=True):
    """got == want on the device, or a failure that names the colours.  order: the cube the frame was ("identity" / "scattered")"""
    import torch
    got, want = got.reshape(N, 3), want.reshape(N, 3)
    if torch.equal(got, want):
        return
    bad = (got != want).any(1).nonzero().flatten()
    first = bad[:8]
    cols = (first if order == "identity" else _dev("perm")[first]).cpu().numpy()
    g, w = got[first].cpu().numpy(), want[first].cpu().numpy()
    if coded:
        g, w = cr.decode(g).tolist(), cr.decode(w).tolist()
    else:
        g, w = [tuple(v) for v in g.tolist()], [tuple(v) for v in w.tolist()]
    pytest.fail(f"{what} on the {order} cube: {bad.numel()} of {N} colours differ from the oracle; {cr.describe_mismatch(cols, g, w)}")


def _ordered(be, frame, P, which, thr):
    if which == "N":
        return be.ordered(frame, P, be.MODE_NEAREST)
    if which == "I":
        return be.ordered(frame, P, be.MODE_IGN, ign_scale=1.0, ign_seed=0)
    return be.ordered(frame, P, be.MODE_MATRIX, thr=thr)


def _odd(frame):
    """the same frame at an odd address (tests/test_gpu_kernels.py: test_unaligned_input_pointer)"""
    import torch
    buf = torch.empty(frame.numel() + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + frame.numel()].view(frame.shape)
    view.copy_(frame)
    assert view.data_ptr() % 2 == 1
    return view


def _coded(gamma, accel, K):
    """Index colours wherever the library admits them.  The accelerator of an INTEGER palette (cell tables, tie codes) is built
    only for 4 colours or more and only when the output bytes are the palette's own colours -- its kernels write the entry they
    hold -- so those cases compare in the palette's colours: every tie between entries of different colour still shows, entries
    of equal colour do not."""
    return gamma or not accel or K < 4


def _want(orc, name, gamma, which, coded):
    """the oracle's answer over the identity cube, in index colours or translated into the palette's own"""
    import torch
    want = _expect(orc, name, gamma, which)
    if coded:
        return want
    out_colors = torch.from_numpy(cr.prepared(orc, name, gamma, coded=False)[1]).cuda()
    return out_colors[want[:, 0].to(torch.int64) | (want[:, 1].to(torch.int64) << 8)]


def _cube_case(be, orc, name, gamma, which, accel=True, odd=False, what=""):
    """One oracle pass, the launches on both cubes (the scattered one where the pass depends on the colour alone), device-side
    comparison with the uploaded expectation."""
    coded = _coded(gamma, accel, len(cr.palette(orc, name)))
    P = be.Palette(*cr.prepared(orc, name, gamma, coded=coded), accel=accel)
    thr = be.Thresholds.from_matrix(np.array(cr.THRESHOLDS[which], np.float32)) if which in cr.THRESHOLDS else None
    want = _want(orc, name, gamma, which, coded)
    for order in ("identity", "scattered") if which in cr.COLOUR_ONLY else ("identity",):
        frame = _dev(order)
        got = _ordered(be, _odd(frame) if odd else frame, P, which, thr)
        _same(got, want if order == "identity" else want[_dev("perm")], order,
              f"{what or 'product library'}: {name} gamma={gamma} pass {which}", coded=coded)


# ==================================================================================================== a. the library that ships
BRUTE_PALETTES = ("two", "palr256", "palr300")    # accel=False: the integer and the float64 brute-force kernels


@pytest.mark.parametrize("which", cr.PASSES)
@pytest.mark.parametrize("gamma", cr.GAMMAS, ids=["int", "gamma"])
@pytest.mark.parametrize("name", list(cr.PALETTES))
def test_product_library(be, orc, name, gamma, which):
    """every palette with its accelerator, as the library chooses tables and kernels itself"""
    _cube_case(be, orc, name, gamma, which)


@pytest.mark.parametrize("which", cr.PASSES)
@pytest.mark.parametrize("gamma", cr.GAMMAS, ids=["int", "gamma"])
@pytest.mark.parametrize("name", BRUTE_PALETTES)
def test_product_library_without_accelerator(be, orc, name, gamma, which):
    _cube_case(be, orc, name, gamma, which, accel=False, what="product library, accel=False")


@pytest.mark.parametrize("gamma", cr.GAMMAS, ids=["int", "gamma"])
def test_product_library_odd_address(be, orc, gamma):
    """frames that are not dword-aligned: the whole-table kernel (integer palette) / the brute-force kernel (use_gamma)"""
    _cube_case(be, orc, "palr256", gamma, "C", odd=True, what="product library, odd address")


# ==================================================================================================== c. the pattern table
PATTERN_PALETTES = [n for n in cr.PALETTES if n not in ("palr300", "palr1024")]     # pattern dithering: at most 256 colours


@pytest.mark.parametrize("gamma", cr.GAMMAS, ids=["int", "gamma"])
@pytest.mark.parametrize("name", PATTERN_PALETTES)
def test_pattern_table_at_every_colour(be, orc, name, gamma):
    """Strength 0 reads the palette's 2^24-entry table at every pixel's own colour: all entries, the brick layout and the
    lut_in path.  The palette's real output colours here: the table stores luminance ranks, and entries of equal colour are
    indistinguishable by the definition in include/ditherpie_hip_pattern.h."""
    import torch
    pal_f32, out_colors, lut_in = cr.prepared(orc, name, gamma, coded=False)
    P = be.Palette(pal_f32, out_colors, lut_in, accel=True)
    coded = _expect(orc, name, gamma, "N")
    idx = coded[:, 0].to(torch.int64) | (coded[:, 1].to(torch.int64) << 8)
    want = torch.from_numpy(out_colors).cuda()[idx]
    for order in ("identity", "scattered"):
        for m in be.PATTERN_MATRICES:
            got = be.pattern(_dev(order), P, m, 0)
            _same(got, want if order == "identity" else want[_dev("perm")], order, f"pattern {m}x{m}, strength 0: {name} gamma={gamma}",
                  coded=False)


# ==================================================================================================== d. error diffusion
ED_PALETTES = ("two", "palr16", "palr256", "clustered200", "mc64", "dup256")
ED_ZERO_TAPS = [(1, 0, 0.0), (-1, 1, 0.0), (0, 1, 0.0), (1, 1, 0.0)]     # the Floyd-Steinberg offsets, nothing pushed
# The cube in the three shapes that reach the three schedules of launch_error_diffusion (ediff.hip), on a device with 256 CUs:
#   one frame of 4096 x 4096    the frame's 64 bands spread over 16 workgroups of two waves (G = 16): the four-wave instance, tables
#                               staged into LDS; the repair launch behind it (sixteen-wave instance) finds nothing to do
#   256 frames of 256 x 256     four bands: one workgroup of four waves per frame, the same four-wave instance without the spread
#   512 frames of 512 x 64      eight bands, more frames than CUs: the sixteen-wave instance on the persistent grid, tables in L2
# With nothing pushed a frame border means nothing, so every shape must give pass N of the same pixels.
ED_SHAPES = ((4096, 4096), (256, 256, 256), (512, 512, 64))
# Which candidate structure answers depends on the palette (K <= 16: the coarse lists of the small-queue instances; 17 .. 256
# colours: the hierarchical H4 table unless the palette is crowded, else the 16^3 lists -- four-wave instances, both in LDS --
# or, sixteen-wave instances, H4 walked in L2 when it is shallow, else the 8^3 cell lists with their octree nodes) and cannot
# be read back from a launch, so test_error_diffusion_forced_structures pins each one with the library's switches.
ED_FORCED = [
    ({"DP_ED_NO_H4": "1"}, "16^3 lists in LDS (four waves) / 8^3 lists with nodes (sixteen waves)"),
    ({"DP_ED_H4_ALWAYS": "1"}, "H4 kept for crowded palettes too: in LDS where it fits (four waves)"),
    ({"DP_ED_H4_ALWAYS": "1", "DP_ED_H4_GLOBAL": "1"}, "H4 walked in L2 by the sixteen-wave instances, shallow or not"),
    ({"DP_ED_H4_LDS_ONLY": "1"}, "the sixteen-wave instances on the 8^3 lists with nodes"),
    ({"DP_ED_TEST_GIVEUP": "1"}, "the spread launch gives up at once: the repair launch (sixteen waves, one workgroup per frame) does the 4096 x 4096 frame"),
]


def _ed_cube(be, orc, name, gamma, serp, shape, what):
    P = be.Palette(*cr.prepared(orc, name, gamma), accel=True)
    want = _expect(orc, name, gamma, "N")
    for order in ("identity", "scattered"):
        got = be.error_diffusion(_dev(order).view(*shape, 3), P, ED_ZERO_TAPS, 16, serp)
        _same(got, want if order == "identity" else want[_dev("perm")], order,
              f"zero-weight error diffusion, frames {shape}, {what}: {name} gamma={gamma} serpentine={serp}")


def _shape_id(shape):
    return "x".join(str(v) for v in shape)


# (serpentine, for one palette, in the 256-frame shape alone: its kernels took 13.8 s over the three shapes on one MI355X)
@pytest.mark.parametrize("name,gamma,serp,shape", [(n, g, False, sh) for n in ED_PALETTES for g in cr.GAMMAS for sh in ED_SHAPES] +
                         [("palr256", False, True, ED_SHAPES[1])],
                         ids=lambda v: _shape_id(v) if isinstance(v, tuple) else None)
def test_error_diffusion_at_every_integer_point(be, orc, name, gamma, serp, shape):
    """With all four weights 0.0 every pixel of an error diffusion is a k=1 query at an integer point (shown with the oracle
    alone in tests/test_colour_cube_cpu.py), so the candidate structures of the diffusion kernels must answer like pass N: the
    cube as the one 4096 x 4096 frame and in the two other shapes of ED_SHAPES, with the structures the library picks itself."""
    _ed_cube(be, orc, name, gamma, serp, shape, "product library")


ED_FORCED_CASES = [(n, g, env, what, sh)
                   for n in ("palr256", "clustered200", "mc64", "dup256")      # 17 .. 256 colours: the palettes with an H4 table
                   for g in cr.GAMMAS for env, what in ED_FORCED for sh in ED_SHAPES
                   # the give-up switch means something to the spread launch only; dup256 (every pixel a tie of twin entries: 12 s
                   # in the repair launch's one workgroup) is left to the other four
                   if "DP_ED_TEST_GIVEUP" not in env or (sh == ED_SHAPES[0] and n != "dup256")]


@pytest.mark.parametrize("name,gamma,env,what,shape", ED_FORCED_CASES,
                         ids=["-".join([n, "gamma" if g else "int", "+".join(k[6:] for k in env), _shape_id(sh)]) for n, g, env, _, sh in ED_FORCED_CASES])
def test_error_diffusion_forced_structures(orc, switches, name, gamma, env, what, shape):
    """The same on the experiments build with the candidate structure pinned (ED_FORCED)."""
    for k, v in env.items():
        switches.setenv(k, v)
    from dither_pie_amd import backend
    _ed_cube(backend, orc, name, gamma, False, shape, f"{env}: {what}")


# ==================================================================================================== e. k-means cell lists
_KM_REF = {}


def _km_centres(K):
    """fractional float64 centres, half of them inside the one 16^3 cell (6, 2, 10)"""
    rs = np.random.RandomState(K)
    return np.concatenate([np.array([96.0, 32.0, 160.0]) + rs.rand(K // 2, 3) * 16, rs.rand(K - K // 2, 3) * 255])


def _km_reference(orc, K, with_mean):
    """orc.kmeans_step over the cube: (sums, counts, sumsq).  The oracle returns no squared norms, so they come from its counts
    over the 3 x 256 planes of the cube: sum of c^2 over a cluster = sum over v of v^2 * (members with c = v), per channel.  (The
    labels depend on the colour alone, so the planes of the first axis also add up to the totals of the whole cube.)"""
    key = (K, with_mean)
    if key not in _KM_REF:
        _dev("identity")
        cube = _HOST["identity"].reshape(256, 256, 256, 3)
        centres = _km_centres(K)
        mean = orc.data_mean(cube) if with_mean else None
        sq = np.arange(256, dtype=np.int64) ** 2
        sums, counts, sumsq = np.zeros((K, 3), np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
        for axis in range(3):
            for v in range(256):
                s, c, _ = orc.kmeans_step(np.ascontiguousarray(np.take(cube, v, axis=axis)).reshape(-1, 3), centres, mean)
                sumsq += sq[v] * c
                if axis == 0:
                    sums += s
                    counts += c
        assert int(counts.sum()) == N and (counts > 0).all()
        _KM_REF[key] = (centres, mean, sums, counts, sumsq)
    return _KM_REF[key]


def _km_check(got, ref, what):
    for name, g, w in zip(("sums", "counts", "sumsq"), got, ref):
        g = g.cpu().numpy()
        assert np.array_equal(g, w), f"k-means {what}: {name} differ from the oracle in clusters {np.argwhere(g != w)[:8, 0].tolist()}"


def _km_args(orc, K, with_mean):
    import torch
    centres, mean, *ref = _km_reference(orc, K, with_mean)
    return torch.from_numpy(centres).cuda(), (torch.from_numpy(mean).cuda() if with_mean else None), ref


@pytest.mark.parametrize("with_mean", (False, True), ids=["lowest-index", "sklearn-ties"])
@pytest.mark.parametrize("K", (16, 64))
def test_kmeans_default_pass(be, orc, K, with_mean):
    centres, mean, ref = _km_args(orc, K, with_mean)
    _km_check(be.kmeans_step(_dev("identity"), centres, mean), ref, f"default pass K={K}")


@pytest.mark.parametrize("with_mean", (False, True), ids=["lowest-index", "sklearn-ties"])
@pytest.mark.parametrize("K", (16, 64))
def test_kmeans_cell_lists(be, orc, switches, K, with_mean):
    switches.setenv("DP_KMEANS_CELLS", "1")
    centres, mean, ref = _km_args(orc, K, with_mean)
    _km_check(be.kmeans_step(_dev("identity"), centres, mean), ref, f"cell lists K={K}")


@pytest.mark.parametrize("with_mean", (False, True), ids=["lowest-index", "sklearn-ties"])
@pytest.mark.parametrize("K", (16, 64))
def test_kmeans_histogram_pass(be, orc, K, with_mean):
    centres, mean, ref = _km_args(orc, K, with_mean)
    hist = be.ColourHistogram(_dev("identity"))
    assert not hist.overflowed()
    _km_check(hist.step(centres, mean), ref, f"histogram pass K={K}")


# ==================================================================================================== b. the experiments library
# (switches, palettes): every pass of cube_ref.PASSES runs for each pair.  Integer palettes unless the name ends in "/gamma";
# "/odd": the frame at an odd address, "/noaccel": the palette without its accelerator.
_T, _ON = "DP_FORCE_TABLE", "1"
FORCED = [
    ({}, ("two", "palr256", "palr300", "palr1024", "dup256", "clustered200", "palr256/odd", "palr256/noaccel", "palr256/gamma", "palr300/gamma",
          "palr256/gamma/odd", "palr256/gamma/noaccel")),
    ({_T: "u4"}, ("uniform27", "palr16", "edges64", "mc64")),                       # u4 needs K <= 64
    ({_T: "u8"}, ("uniform27", "palr256", "mc64", "mc64/odd")),
    ({_T: "w4"}, ("uniform27", "palr16", "palr300")),                              # the warped tables need K >= 8
    ({_T: "w8"}, ("uniform27", "palr256", "palr300", "mc256")),
    ({"DP_FORCE_COMPACT": _ON}, ("uniform27", "uniform125", "palr256")),
    ({"DP_FORCE_COMPACT": _ON, "DP_COMPACT_NO_HALF": _ON}, ("uniform125",)),
    ({_T: "w8", "DP_FORCE_COMPACT": _ON}, ("palr256",)),
    ({_T: "w8", "DP_FORCE_COMPACT": _ON, "DP_COMPACT_NO_HALF": _ON}, ("palr256",)),
    ({"DP_COMPACT_NO_HALF": _ON}, ("dup256", "clustered200", "mc64")),              # palettes that take the compact kernel by themselves
    ({"DP_NO_COMPACT_KERNEL": _ON}, ("dup256", "clustered200", "mc64", "mc256", "uniform125/gamma", "palr256/gamma", "mc64/gamma")),
    ({"DP_LEAN_NO_HALF": _ON}, ("uniform27",)),
    ({"DP_NO_FAST": _ON}, ("uniform27", "uniform125", "palr256")),
    ({"DP_NO_FAST": _ON, "DP_LEAN_NO_HALF": _ON}, ("uniform27",)),
    ({"DP_FAST_ALL": _ON}, ("uniform27", "uniform125", "palr256")),
    ({"DP_NO_WARP": _ON}, ("palr16", "clustered200", "mc64")),
]
CASES = [(spec.split("/")[0], "gamma" in spec.split("/"), env, which, next((k for k in ("odd", "noaccel") if k in spec.split("/")), ""))
         for env, specs in FORCED for spec in specs for which in cr.PASSES]
CASES.sort(key=lambda c: (list(cr.PALETTES).index(c[0]), c[1], cr.PASSES.index(c[3])))   # cases that share an oracle pass run back to back

# Pass-1 kernels of KERNELS that no real palette reaches at this frame size, each with the condition of plan_ordered or accel.hip
# that rules it out.  Empty: the cases above reach all 66 instantiations the launcher names.
UNREACHED = {}

TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) \(4-byte aligned frames: (\d)\) mode=(\d) bw=(\d) adapt=(\d) warp=(\d) half=(\d) "
                   r"table=(\w+) fix_big_queue=(\d)")
_REACHED = {}   # case id -> ((family, MODE, BW, ADAPT, WARP, HALF), table, fix_big_queue) as traced


def _case_id(case):
    name, gamma, env, which, kind = case
    return "-".join([name, "gamma" if gamma else "int", "+".join(f"{k[3:]}={v}" for k, v in env.items()) or "noswitch", which] + [kind] * bool(kind))


def _traced(capfd, launches):
    """the one instantiation the launches since the last readouterr() ran"""
    seen = TRACE.findall(capfd.readouterr().err)
    assert len(seen) == launches and len(set(seen)) == 1, seen
    fam, _, mode, bw, adapt, warp, half, table, big = seen[0]
    return (fam, int(mode), int(bw), int(adapt), int(warp), int(half)), table, int(big)


def _forced(switches, env):
    for k, v in env.items():
        switches.setenv(k, v)
    switches.setenv("DP_ORDERED_TRACE", "1")
    from dither_pie_amd import backend
    return backend


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_forced_tables_and_kernels(orc, switches, capfd, case):
    """The comparison of part a with the table and the kernel forced by switches; which instantiation ran is recorded for
    test_cube_cases_cover_the_kernels."""
    name, gamma, env, which, kind = case
    be = _forced(switches, env)
    capfd.readouterr()
    _cube_case(be, orc, name, gamma, which, accel=kind != "noaccel", odd=kind == "odd", what=f"experiments library {env} {kind}")
    _REACHED[_case_id(case)] = _traced(capfd, 2 if which in cr.COLOUR_ONLY else 1)


def test_cube_cases_cover_the_kernels(orc, switches, capfd):
    """The traced (family, MODE, BW, ADAPT, WARP, HALF) of all cases of test_forced_tables_and_kernels are KERNELS
    (tests/test_ordered_plan_cpu.py: every pass-1 instantiation the launcher names) minus UNREACHED, and nothing of UNREACHED
    was reached; both sizes of the fix-up queue were used.  A case that did not run in this session (a selection with -k) is
    launched here, without the comparison, for its trace line alone."""
    for case in CASES:
        if _case_id(case) in _REACHED:
            continue
        name, gamma, env, which, kind = case
        with pytest.MonkeyPatch.context() as mp:
            be = _forced(mp, env)
            accel = kind != "noaccel"
            P = be.Palette(*cr.prepared(orc, name, gamma, coded=_coded(gamma, accel, len(cr.palette(orc, name)))), accel=accel)
            thr = be.Thresholds.from_matrix(np.array(cr.THRESHOLDS[which], np.float32)) if which in cr.THRESHOLDS else None
            capfd.readouterr()
            _ordered(be, _odd(_dev("identity")) if kind == "odd" else _dev("identity"), P, which, thr)
            _REACHED[_case_id(case)] = _traced(capfd, 1)
            del P, thr
    reached = {}
    for cid, (key, table, _) in sorted(_REACHED.items()):
        reached.setdefault(key, []).append(f"{cid} [{table}]")
    with capfd.disabled():
        print("\npass-1 kernels the cube cases reached (family, MODE, BW, ADAPT, WARP, HALF):")
        for key in sorted(reached):
            print(f"  {key}: {len(reached[key])} cases, e.g. {reached[key][0]}")
    assert set(UNREACHED) <= KERNELS and all(reason.strip() for reason in UNREACHED.values())
    assert not set(reached) - KERNELS, sorted(set(reached) - KERNELS)
    assert not set(reached) & set(UNREACHED), f"listed as unreachable but reached: {sorted(set(reached) & set(UNREACHED))}"
    assert set(reached) == KERNELS - set(UNREACHED), f"no cube case reached {sorted(KERNELS - set(UNREACHED) - set(reached))}"
    # what UNREACHED may never hold
    left = KERNELS - set(UNREACHED)
    assert {k[0] for k in left} == {k[0] for k in KERNELS}                                       # no whole family
    assert {k for k in KERNELS if k[0] in ("lean", "compact") and k[1] in (0, 1)} <= left       # every lean / compact shape, MODE 0 and 1
    assert {k for k in KERNELS if k[0] == "fast" and k[1] == 0} <= left                          # both BW of the fast kernel
    for fam in {k[0] for k in KERNELS}:
        for mode in {k[1] for k in KERNELS if k[0] == fam} & ({1, 2, 3} if fam == "fast" else {2, 3}):
            assert any(k[0] == fam and k[1] == mode for k in left), (fam, mode)
    assert {big for _, _, big in _REACHED.values()} == {0, 1}, "one size of the fix-up queue was never used"
