"""The whole colour cube as a test input (no GPU in here): all 2^24 colours as one 4096 x 4096 frame, in identity order and
in a scattered order, the named palettes the cube tests run, output colours that spell the chosen palette index, and the
passes -- each answered by the CPU oracle (oracle/oracle.py: ordered_u8) -- whose results the device must reproduce colour
by colour.  tests/test_colour_cube_cpu.py checks the helper itself; tests/test_gpu_colour_cube.py uses it."""
import functools

import numpy as np

SIDE = 4096
N = 1 << 24
# scattered order: pixel p holds colour (p * M) mod 2^24.  M is odd, so the map is a bijection of the cube; its high and low
# bits are set (the golden-ratio multiplier of 24 bits), so the four pixels of a group and the 64 lanes of a wave fall into
# unrelated 16^3 cells
M = 0x9E3779
PASSES = ("N", "S", "F", "C", "I")
COLOUR_ONLY = ("N", "S", "F")     # passes that do not depend on the position: what the scattered cube is compared for
# thresholds of the matrix passes.  0 sends every colour with d0 > 0 to the second entry of the k=2 query; 2^-20 lies below
# the smallest non-zero factor d0 / (d0 + d1) of an integer palette (1 / 195076), so it decides like 0 but has no integer form
# and runs the float32-threshold kernels; the 2x2 checkerboard mixes slots that can only take the nearest entry with full ones
THRESHOLDS = {"S": [[0.0]], "F": [[2.0 ** -20]], "C": [[0.0, 1.0], [1.0, 0.0]]}


def colours_of(p):
    """[..., 3] uint8 colours of the 24-bit colour numbers p"""
    p = np.asarray(p, dtype=np.int64)
    return np.stack([p >> 16, (p >> 8) & 255, p & 255], -1).astype(np.uint8)


def scatter_index():
    """perm[p] = (p * M) mod 2^24: the colour number pixel p of the scattered cube holds (int64 [2^24])"""
    return (np.arange(N, dtype=np.int64) * M) & (N - 1)


def identity_cube():
    return colours_of(np.arange(N, dtype=np.int64)).reshape(SIDE, SIDE, 3)


def scattered_cube():
    return colours_of(scatter_index()).reshape(SIDE, SIDE, 3)


def gather(identity_result, perm=None):
    """What a colour-only operation gives on the scattered cube, from its result on the identity cube: pixel p of the
    scattered cube holds colour perm[p], whose result is pixel perm[p] of the identity result."""
    perm = scatter_index() if perm is None else perm
    flat = identity_result.reshape(N, -1)
    return flat[perm].reshape(identity_result.shape)


# ------------------------------------------------------------------------------------------------------ output colours
def index_colours(K):
    """out_colors[k] = (k & 255, k >> 8, 0): the output bytes are the chosen index, so entries of equal colour differ too"""
    k = np.arange(K)
    return np.ascontiguousarray(np.stack([k & 255, k >> 8, np.zeros_like(k)], -1).astype(np.uint8))


def decode(out):
    """the palette indices an output in index colours spells (int32 [...]): out[..., 2] must be 0"""
    assert not out[..., 2].any()
    return out[..., 0].astype(np.int32) | (out[..., 1].astype(np.int32) << 8)


# ------------------------------------------------------------------------------------------------------ palettes
def _clustered(orc, K, seed):
    """as tests/fuzz_ordered.py makes them: four fifths of the entries inside one 6-wide cube, the rest anywhere"""
    rs = np.random.RandomState(seed)
    c0 = rs.randint(20, 200, 3)
    nd = (K * 4) // 5
    return [tuple(int(v) for v in c0 + rs.randint(0, 6, 3)) for _ in range(nd)] + orc.palr(K - nd, seed + 1)


def _median_cut(orc, kind, K):
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    return [tuple(int(v) for v in c) for c in ColorReducer.reduce_colors(Image.fromarray(orc.imgl(120, 203, 5, kind), "RGB"), K)]


PALETTES = {
    "one": lambda orc: [(90, 160, 33)],
    "two": lambda orc: [(0, 0, 0), (2, 0, 0)],
    "uniform27": lambda orc: orc.generate_uniform_palette(27),      # lattice bisector planes through integer points
    "uniform125": lambda orc: orc.generate_uniform_palette(125),
    "edges64": lambda orc: [(r, g, b) for r in (15, 16, 127, 128) for g in (15, 16, 127, 128) for b in (15, 16, 127, 128)],
    "palr16": lambda orc: orc.palr(16, 11),
    "palr256": lambda orc: orc.palr(256, 21),
    "palr300": lambda orc: orc.palr(300, 2),
    "palr1024": lambda orc: orc.palr(1024, 5),
    "dup256": lambda orc: orc.palr(128, 13) * 2,
    "clustered200": lambda orc: _clustered(orc, 200, 17),
    "mc64": lambda orc: _median_cut(orc, "smooth", 64),
    "mc256": lambda orc: _median_cut(orc, "dark", 256),
}
GAMMAS = (False, True)


@functools.lru_cache(maxsize=None)
def _palette(orc, name):
    return tuple(PALETTES[name](orc))


def palette(orc, name):
    """the named palette as a list of (r, g, b)"""
    return list(_palette(orc, name))


def prepared(orc, name, gamma, coded=True):
    """(pal_f32, out_colors, lut_in) of the named palette; coded: index colours instead of the palette's own"""
    pal_f32, out_colors, lut_in = orc.prepare_palette(palette(orc, name), gamma)
    return pal_f32, (index_colours(len(pal_f32)) if coded else out_colors), lut_in


# ------------------------------------------------------------------------------------------------------ the passes
def oracle_pass(orc, arr, pal_f32, out_colors, lut_in, which):
    """One pass of the oracle over the frame `arr` (whose first pixel is the origin)."""
    if which == "N":
        return orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "none")
    if which == "I":
        return orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "ign", scale=1.0, seed=0)
    return orc.ordered_u8(arr, pal_f32, out_colors, lut_in, "matrix", thr=np.array(THRESHOLDS[which], np.float32))


def expected(orc, name, gamma, which, cube=None):
    """The oracle's output in index colours of pass `which` over the identity cube, [4096, 4096, 3] uint8."""
    cube = identity_cube() if cube is None else cube
    return oracle_pass(orc, cube, *prepared(orc, name, gamma), which)


# ------------------------------------------------------------------------------------------------------ reporting
def describe_mismatch(colour_numbers, got, want, limit=8):
    """colour_numbers: the 24-bit colours of the mismatching pixels, got / want their decoded indices (or output colours)"""
    lines = []
    for c, g, w in list(zip(colour_numbers, got, want))[:limit]:
        r, gg, b = int(c) >> 16, (int(c) >> 8) & 255, int(c) & 255
        lines.append(f"colour ({r},{gg},{b}) cell ({r >> 4},{gg >> 4},{b >> 4}): device {g}, oracle {w}")
    return "; ".join(lines)
