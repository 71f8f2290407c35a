"""Steered queries for the nearest-colour search of the diffusion kernels (no GPU in here).

Every diffusion kernel asks, per pixel, which palette entry is nearest to a float32 point: the pixel plus the error pushed
into it.  This module builds frames in which ONE known push reaches every pixel of interest, so that the point a chosen pixel
asks about is a chosen float32 point, predicts those points in float32 as the oracle computes them, and picks the points that
matter.  tests/test_steer_cpu.py pins the prediction against the points the oracle reports (oracle.py: want_queries) and
checks the floors below from that report; tests/test_gpu_steered_queries.py launches the frames.

Donor dictionary.  The oracle's pass N over the identity cube gives, for every colour A, e(A) = f32(lut_in[A] or A) -
pal_f32[nearest(A)]; one donor colour is kept per distinct error vector (distinct by a 64-bit hash of the three floats).

Layouts (all arithmetic float32 in the oracle's order; a receiver asks about B' + fl32(e(A) * w), B' = f32(lut_in[B] or B)):
  pair      rows [donor, receiver] of frames (N, H, 2) with the single tap (1, 0, w): every row is on its own; under serpentine
            the donor of an odd row sits at x = 1.  error_diffusion (both arithmetics, both scans) and Ostromoukhov with a
            coefficient table whose rows are {w, 0, 0}; the query is clamped to [0, 255].
  tile      adaptive variance with an explicit gate: 2 x 3 tiles [idle, D, R] over [R, R, R], the gate set on D only; the four
            receivers get e(D) times 7/16 (right), 3/16, 5/16, 1/16 (below, left to right); unclamped.  One receiver of a tile
            is the target, the other three hold the same colour and ask about whatever that gives.
  pair1     frames (N, 1, 2) for the perceptual and the hybrid diffuser: only the right tap stays in the frame; unclamped.  Their
            pushes (a weight that follows the donor's luminance; a linear map of the error) are searched for the ladder too.
  saturate  whole frames far from the palette's hull, every gate on; nothing is predicted, the oracle judges and its report
            measures how far beyond the cube the queries went.

Targets, grouped by weight (one launch has one weight): 2^-1 .. 2^-16 for the pair layout, the tile's four for the tile.
  gap     every 16^3 cell gets, per weight, one query per axis whose integer part is the LAST of the cell on that axis
          (16c + 15) with a non-zero fraction -- the points between a cell's last integer and its face, which no integer test
          visits -- and one more fractional query.  Where the kernel clamps, 255.x does not exist and the last integer part
          of the cells 15 is 254.  The same for LEAVES 2-wide leaves (last integer part 2l + 1), half of them around palette
          entries, where the hierarchical table descends that far.
  face    clamped layouts: one, two or three coordinates exactly 0.0 or 255.0, the others fractional: all 26 faces, edges and
          corners, each by OVERSHOOT (the value before the clamp lies beyond the face) in every direction the palette's errors
          point in -- all 26 but for `two`, whose errors are never negative (NO_NEGATIVE_ERROR): its faces at 0 are reached from
          pixels on them.
  ladder  near ties.  Pairs (i, j) of DISTINCT colours that are nearest and second nearest of some colour (a k = 2 query over
          a sample of the cube; the PAIRS_TRIED tried are the most distant ones and a random draw of the rest).  For each pair
          the search space is: of the 11 reachable B' nearest the midpoint per axis the 125 points nearest the bisector plane,
          the donors with |e|inf <= 6 (at most POOL of them), every weight.  Per B', weight and rung the two donors whose push
          comes nearest the rung's centre are evaluated: the query in float32, its relative gap (d1 - d0) / d0 from the float64
          squared distances; a float64 scan over the whole palette then confirms that i and j are the global top two.  The rungs start at float32's epsilon and are deliberately not
          the kernels' margins (2e-6 .. 4e-6): they straddle any margin in that range from both sides.  Entries of equal colour
          (dup256) count as one colour here: between twins every gap is 0.
  out     tile and pair1: queries beyond the cube in all 26 directions at distances near 1, 16, 64 and >= 100 -- as far as the
          palette's largest errors carry: a push of e * 7/16 reaches 100 only where some colour is 229 from its entry.

Floors (asserted in the CPU tier from the oracle's report, never from device output): gap and face in full for every palette;
per rung, queries from at least min(20, a tenth of the adjacent pairs, >= 1) distinct pairs, at least half of them fractional,
the exact-tie rung for integer palettes only -- for the pair layout, the tile layout and the pair1 frames of PAIR1_CASES alike, each
with the pushes it really makes.  A (layout, palette) that misses a rung's floor has the count this search finds recorded in
LADDER_RECORDED below, with the reason, and that count is asserted instead.

Generator cost (dictionary + targets, cached per palette and use_gamma): 9 to 17 s of WALL time per palette on 8 cores (the
oracle's pass over the cube runs on all of them: process CPU time is 11 to 22 s), about
7 s of it the dictionary (the oracle's pass over the cube and the sort of 2^24 error vectors): GENERATOR_SECONDS at the end of
the module.  Above the ~10 s aimed at the pairs were cut (24 kept per rung of 160 tried), not the rungs."""
import functools
import time

import numpy as np

import cube_ref as cr

F = np.float32
PALETTES = ("two", "palr16", "mc64", "clustered200", "dup256", "palr256", "palr300", "palr1024")
PAIR_WEIGHTS = tuple(2.0 ** -k for k in range(1, 17))
TILE_WEIGHTS = (7.0 / 16, 3.0 / 16, 5.0 / 16, 1.0 / 16)      # receivers (0, 2), (1, 0), (1, 1), (1, 2) of a tile
TILE_SLOTS = ((0, 2), (1, 0), (1, 1), (1, 2))
RUNGS = ((0.0, 0.0), (0.0, 1e-7), (1e-7, 1e-6), (1e-6, 4e-6), (4e-6, 1e-5), (1e-5, 1e-4))     # (lo, hi]: lo < gap <= hi; the first: gap == 0
RUNG_NAMES = ("exact tie", "(0, 1e-7]", "(1e-7, 1e-6]", "(1e-6, 4e-6]", "(4e-6, 1e-5]", "(1e-5, 1e-4]")
KINDS = ("filler", "gap16", "gap2", "face", "ladder", "out")
K_FILLER, K_GAP16, K_GAP2, K_FACE, K_LADDER, K_OUT = range(6)
LEAVES = 512          # 2-wide leaves sampled for the gap targets
POOL = 4096           # donors with |e|inf <= 6 the ladder search and the gap / face solvers draw from
PAIRS_TRIED = 160     # adjacent pairs the ladder search tries per palette
PAIRS_KEPT = 24       # ... and keeps per rung (three queries each)
OUT_DISTANCES = (1.0, 16.0, 64.0, 100.0)
# (distance beyond the cube, least push of the donor): (1, 16) is a receiver just outside whose tile mates, with their smaller
# weights, stay inside -- the one outside lane of a band
OUT_TARGETS = ((1.0, 1.0), (1.0, 16.0), (16.0, 16.0), (64.0, 64.0), (100.0, 100.0))
DIRECTIONS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]

# the perceptual / hybrid cases both tiers run (pair1 layout): palettes of every size class, both use_gamma values
PAIR1_CASES = (("two", False), ("palr16", True), ("mc64", False), ("palr256", True), ("dup256", False), ("palr1024", False))
PAIR1_FRAMES = 2048
# (layout, palette, use_gamma) -> {rung index: distinct pairs found}, for the rungs whose floor the palette misses in that layout;
# the CPU tier asserts exactly these counts from the oracle's report, and the floor for everything not listed.  The counts are
# what the search described above finds in its space (for `two`, tests/test_steer_cpu.py also enumerates the whole space).
#   pair, tile on INTEGER palettes: the query is B + e * w with integers B and e, so the gap d1 - d0 = 2 (q - mid) . (p_i - p_j) moves in
#     steps of 2^-15 (pair, w = 2^-16) or 1/8 (tile, w = k/16).  A step of 1/8 is more than 1e-4 of any d0 below 1250: the tile
#     reaches exact ties and, for distant pairs, the top rung, nothing between.  One step of 2^-15 is more than 1e-7 of the d0
#     that `two` (below 340 this near its one midpoint) and `mc64` (neighbours a few units apart) offer.
#   `two` under use_gamma: entries 0 and 0.155 on r, so B' = 0 and a push of 0.077, which few errors times a weight come near.
#   pair1: the perceptual / hybrid pushes are fine-grained but not free; where fewer pairs than the floor are found the count stands.
LADDER_RECORDED = {
    ("pair", "mc64", False): {1: 0},
    ("pair", "two", False): {1: 0},
    ("pair", "two", True): {1: 0, 2: 0},
    ("pair1-1", "dup256", False): {1: 16},
    ("pair1-1", "mc64", False): {1: 0, 2: 19},
    ("pair1-1", "palr1024", False): {1: 14},
    ("pair1-1", "two", False): {1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
    ("pair1-2", "dup256", False): {1: 3},
    ("pair1-2", "mc64", False): {1: 0, 2: 1, 3: 9, 4: 14},
    ("pair1-2", "palr1024", False): {1: 3, 2: 13},
    ("pair1-2", "two", False): {1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
    ("tile", "clustered200", False): {1: 0, 2: 0, 3: 0, 4: 0},
    ("tile", "dup256", False): {1: 0, 2: 0, 3: 0, 4: 0},
    ("tile", "mc64", False): {1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
    ("tile", "mc64", True): {1: 15},
    ("tile", "palr1024", False): {1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
    ("tile", "palr16", False): {1: 0, 2: 0, 3: 0, 4: 0},
    ("tile", "palr256", False): {1: 0, 2: 0, 3: 0, 4: 0},
    ("tile", "palr300", False): {1: 0, 2: 0, 3: 0, 4: 0},
    ("tile", "two", False): {1: 0, 2: 0, 3: 0, 4: 0, 5: 0},
    ("tile", "two", True): {1: 0, 2: 0, 3: 0, 4: 0},
}

# (layout, palette, use_gamma) -> fractional queries on the exact-tie rung, where they are fewer than half of that rung's queries.
# An exact tie at a fractional point needs a push exactly perpendicular to p_i - p_j.  Powers of two and sixteenths times an integer
# error give that; the perceptual weight (a float32 function of the donor's luminance) gives it for some pairs, and the hybrid
# push (a float32 mix of all three channels) only when the error is 0 and the point an integer one.
TIE_FRACTIONAL_RECORDED = {
    ("pair1-2", "two", False): 0, ("pair1-2", "mc64", False): 0, ("pair1-2", "dup256", False): 0, ("pair1-2", "palr1024", False): 0,
    ("pair1-1", "dup256", False): 12, ("pair1-1", "palr1024", False): 14,
}


@functools.lru_cache(maxsize=1)
def _cube():
    return cr.identity_cube()


def _lum_f32(v):
    """(0.299 * r + 0.587 * g) + 0.114 * b in float32, every operation rounded"""
    return (F(0.299) * v[..., 0] + F(0.587) * v[..., 1]) + F(0.114) * v[..., 2]


class Steer:
    """Dictionary and targets of one (palette, use_gamma)."""

    def __init__(self, orc, name, gamma):
        t0 = time.perf_counter()
        self.orc, self.name, self.gamma = orc, name, gamma
        self.pal, self.out_colors, self.lut = cr.prepared(orc, name, gamma)
        self.K = len(self.pal)
        lut = self.lut if self.lut is not None else np.arange(256, dtype=np.uint8)
        self.V, self.rep = np.unique(lut, return_index=True)       # reachable B' values and a pixel value that gives each
        self.V = self.V.astype(F)
        self.rep = self.rep.astype(np.uint8)
        self._dictionary()
        self.rows = {}        # ("pair" | "tile", weight index) -> dict(A, B, e, kind, rung, pair)
        self.ladder_stats = None
        self._targets()
        # what stays: the far donors (pair1_frames, and the reach the CPU tier reads); the dictionary itself is up to 250 MB
        self.n_donors = len(self.donor_A)
        self.far_A, self.far_e = self.donor_A[self.far], self.donor_e[self.far]
        self.pool_A, self.pool_e = self.donor_A[self.pool], self.donor_e[self.pool]
        del self.donor_A, self.donor_e, self.pool, self.far
        self.seconds = time.perf_counter() - t0

    # -------------------------------------------------------------------------------------------------- dictionary
    def src(self, px):
        """f32(lut_in[px] or px)"""
        return (self.lut[px] if self.lut is not None else px).astype(F)

    def _dictionary(self):
        cube = _cube().reshape(-1, 3)
        idx = cr.decode(cr.expected(self.orc, self.name, self.gamma, "N", _cube())).reshape(-1)
        err = self.src(cube) - self.pal[idx]
        bits = np.ascontiguousarray(err).view(np.uint32).astype(np.uint64)
        key = bits[:, 0] * np.uint64(0x9E3779B97F4A7C15) ^ bits[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F) ^ bits[:, 2] * np.uint64(0x165667B19E3779F9)
        _, first = np.unique(key, return_index=True)
        self.donor_A = np.ascontiguousarray(cube[first])
        self.donor_e = np.ascontiguousarray(err[first])
        rs = np.random.RandomState(len(first) & 0xffff)
        small = np.flatnonzero(np.abs(self.donor_e).max(1) <= 6)          # (the colours that are palette entries, e = 0, among them)
        if len(small) > POOL:
            small = np.sort(rs.choice(small, POOL, replace=False))
        self.pool = small
        # the far donors: a random sample of the dictionary, the six single-axis extremes of all of it, and per direction the
        # donors of the sample that carry furthest
        samp = np.sort(rs.choice(len(first), min(len(first), 200000), replace=False))
        samp = np.unique(np.concatenate([samp, self.donor_e.argmax(0), self.donor_e.argmin(0)]))
        es = self.donor_e[samp]
        far = [samp[:20000:1] if len(samp) <= 20000 else samp[rs.choice(len(samp), 20000, replace=False)]]
        for d in DIRECTIONS:
            dd = np.array(d, F)
            reach = np.where(dd != 0, es * dd, np.inf).min(1)           # the smallest component along the direction's axes
            far.append(samp[np.argpartition(-reach, min(64, len(reach) - 1))[:64]])
        self.far = np.unique(np.concatenate(far))

    # -------------------------------------------------------------------------------------------------- pushes
    def push_pair(self, e, w):
        return e * F(w)

    def push_model1(self, A, e):
        """PerceptualDitherStrategy's right tap: e * (7/16 * (0.5 + 0.5 * lum / 255)), lum of the donor's source pixel"""
        scale = F(0.5) + F(0.5) * (_lum_f32(self.src(A)) / F(255.0))
        return e * (F(7.0 / 16) * scale)[..., None]

    def push_model2(self, e, lf=1.0, cf=0.2):
        """HybridDitherStrategy's right tap"""
        lv = _lum_f32(e)
        el = np.stack([F(0.299) * lv, F(0.587) * lv, F(0.114) * lv], -1)
        fe = F(lf) * el + F(cf) * (e - el)
        return fe * F(7.0 / 16)

    def error_of(self, A):
        """e(A) for donor colours [n, 3] (one oracle query each)"""
        src = self.src(A)
        _, ii = self.orc.Tree(self.pal).query(src.astype(np.float64), 1)
        return src - self.pal[ii[:, 0]]

    # -------------------------------------------------------------------------------------------------- solvers
    def _axis_tables(self, d, width, clamp):
        """per donor m, axis a and cell coordinate c: an index into V that puts the query into cell c (any_v) / onto the last
        integer part of cell c with a non-zero fraction (edge_v); -1 where there is none"""
        M = len(d)
        nc = 256 // width
        any_v = np.full((M, 3, nc), -1, np.int32)
        edge_v = np.full((M, 3, nc), -1, np.int32)
        m_rank = np.arange(M)
        for a in range(3):
            Q = self.V[None, :] + d[:, a, None]                      # float32 sum, [M, |V|]
            if clamp:
                Q = np.clip(Q, F(0), F(255))
            ip = np.floor(Q)
            inside = (Q >= 0) & (Q < 256) & (Q != ip)
            cell = np.clip(ip, 0, 255).astype(np.int32) // width
            for c in range(nc):
                last = width * c + width - 1
                if clamp and last == 255:
                    last = 254
                for table, mask in ((any_v, inside & (cell == c)), (edge_v, inside & (ip == last))):
                    cnt = mask.sum(1)
                    order = np.cumsum(mask, 1)
                    want = (m_rank % np.maximum(cnt, 1)) + 1              # a different choice per donor
                    v = np.argmax(mask & (order == want[:, None]), 1)
                    table[:, a, c] = np.where(cnt > 0, v, -1)
        return any_v, edge_v

    def _solve_cells(self, A, e, d, width, cells, clamp, kind, free=1):
        """rows (A, B) whose receiver's query lies in each cell of `cells` [C, 3]: one per axis on the last integer part, `free`
        more anywhere in the cell"""
        any_v, edge_v = self._axis_tables(d, width, clamp)
        M, C = len(d), len(cells)
        num = np.arange(C)
        out_m, out_v = [], []
        for variant in range(3 + free):
            tabs = [edge_v if a == variant else any_v for a in range(3)]
            vs = np.stack([tabs[a][:, a, :][:, cells[:, a]] for a in range(3)], -1)        # [M, C, 3]
            ok = (vs >= 0).all(-1)
            rank = np.where(ok, (np.arange(M)[:, None] - num[None, :] * 7 - variant * 3) % M, M + 1)
            m = rank.argmin(0)
            good = ok[m, num]
            out_m.append(m[good])
            out_v.append(vs[m, num][good])
        m, v = np.concatenate(out_m), np.concatenate(out_v)
        return dict(A=A[m], e=e[m], B=self.rep[v], kind=np.full(len(m), kind, np.uint8))

    def _solve_face(self, A, e, d):
        """clamped layouts: the 26 faces, edges and corners; free axes fractional and inside"""
        rs = np.random.RandomState(5)
        rows = []
        frac = d != np.floor(d)
        for dirn in DIRECTIONS:
            dd = np.array(dirn)
            sign_ok = ((dd == 0) & frac) | ((dd > 0) & (d >= 0)) | ((dd < 0) & (d <= 0))
            cand = np.flatnonzero(sign_ok.all(1))
            # overshooting donors first
            over = (((dd > 0) & (d > 0)) | ((dd < 0) & (d < 0)) | (dd == 0))[cand].all(1)
            cand = np.concatenate([cand[over], cand[~over]])[:6]
            for m in cand:
                v = np.empty(3, np.int64)
                for a in range(3):
                    if dd[a] > 0:
                        v[a] = len(self.V) - 1
                    elif dd[a] < 0:
                        v[a] = 0
                    else:
                        q = self.V + d[m, a]
                        okv = np.flatnonzero((q > 0) & (q < 255) & (q != np.floor(q)))
                        if not len(okv):
                            break
                        v[a] = okv[rs.randint(len(okv))]
                else:
                    rows.append((m, v))
        if not rows:
            return None
        m = np.array([r[0] for r in rows])
        v = np.stack([r[1] for r in rows])
        return dict(A=A[m], e=e[m], B=self.rep[v], kind=np.full(len(m), K_FACE, np.uint8))

    def _solve_out(self, A, e, d):
        """unclamped layouts: queries beyond the cube, per direction and distance, as far as these pushes carry"""
        rs = np.random.RandomState(9)
        rows = []
        for dirn in DIRECTIONS:
            dd = np.array(dirn)
            on = dd != 0
            along = np.where(on, d * dd, np.inf)                      # how far each donor pushes along the direction's axes
            reach = along.min(1)
            for dist, least in OUT_TARGETS:
                cand = np.flatnonzero(reach >= least)
                if not len(cand):
                    continue
                # the donors that overshoot least above the wanted distance come first: B' can then sit on the face's side.  Every
                # coordinate that leaves the cube does so by [dist, 2 * dist) (by at least 100 for the last class): B' is the
                # reachable value that gives the smallest such overshoot, and a donor with none is passed over
                hi = np.inf if dist >= OUT_DISTANCES[-1] else 2 * dist
                cand = cand[np.argsort(reach[cand], kind="stable")][:40]
                taken = 0
                for m in cand:
                    v = np.empty(3, np.int64)
                    for a in range(3):
                        q = self.V + d[m, a]                                 # float32, as the oracle adds
                        over = q - F(255) if dd[a] > 0 else -q
                        okv = np.flatnonzero((over >= dist) & (over < hi)) if dd[a] != 0 else np.flatnonzero((q > 0) & (q < 255))
                        if not len(okv):
                            break
                        v[a] = okv[np.argmin(over[okv])] if dd[a] != 0 else okv[rs.randint(len(okv))]
                    else:
                        rows.append((m, v))
                        taken += 1
                        if taken == 3:
                            break
        if not rows:
            return None
        m = np.array([r[0] for r in rows])
        v = np.stack([r[1] for r in rows])
        return dict(A=A[m], e=e[m], B=self.rep[v], kind=np.full(len(m), K_OUT, np.uint8))

    # -------------------------------------------------------------------------------------------------- ladder
    def b_candidates(self, mid, n):
        """B' of the ladder's search space for a pair with midpoint `mid` and difference `n`: of the 11 reachable values nearest the
        midpoint per axis, the 125 points nearest the bisector plane, as indices into V [125, 3]"""
        V64 = self.V.astype(np.float64)
        near = [np.argsort(np.abs(V64 - mid[a]), kind="stable")[:min(11, len(V64))] for a in range(3)]
        vi = np.stack(np.meshgrid(*near, indexing="ij"), -1).reshape(-1, 3)
        off = V64[vi] - mid
        return vi[np.lexsort(((off ** 2).sum(1), np.abs(off @ n)))[:125]]

    def _ladder(self, groups):
        """groups: [(key, d [M, 3] float32 pushes of the pool's donors, clamp)].  -> {key: rows}, and self.ladder_stats"""
        orc = self.orc
        upal, first = np.unique(self.pal.astype(np.float64), axis=0, return_index=True)
        Ku = len(upal)
        stats = dict(adjacent=0, floor=1, pairs=[0] * len(RUNGS), queries=[0] * len(RUNGS), fractional=[0] * len(RUNGS))
        self.ladder_stats = stats
        found = {key: [] for key, _, _ in groups}
        if Ku < 2:
            return found
        rs = np.random.RandomState(3)
        sample = np.concatenate([rs.randint(0, 256, (40000, 3)), np.clip(np.rint(upal), 0, 255).astype(np.int64)])
        sample = self.src(sample.astype(np.uint8)).astype(np.float64)
        _, ii = orc.Tree(upal).query(sample, 2)
        pairs = np.unique(np.sort(ii, 1), axis=0)
        stats["adjacent"] = len(pairs)
        stats["floor"] = min(20, max(1, len(pairs) // 10))
        # the tried pairs: the most distant ones first (a gap of one step of the finest weight is the smaller a fraction of d0
        # the further the two colours are apart), the rest drawn at random
        apart = ((upal[pairs[:, 0]] - upal[pairs[:, 1]]) ** 2).sum(1)
        by_dist = np.argsort(-apart, kind="stable")
        head = by_dist[:PAIRS_TRIED * 5 // 8]
        rest = by_dist[PAIRS_TRIED * 5 // 8:]
        pairs = pairs[np.concatenate([head, rest[rs.permutation(len(rest))[:PAIRS_TRIED - len(head)]]])]
        centres = np.array([0.0] + [s * np.sqrt(max(lo, hi / 4) * hi) for lo, hi in RUNGS[1:] for s in (1, -1)])
        # layout family -> rung -> {pair number: [(key, donor m, B value indices, fractional)]}: every layout keeps its own pairs
        fams = sorted({key if key[0] == "pair1" else key[:1] for key, _, _ in groups})
        fam_of = np.array([fams.index(key if key[0] == "pair1" else key[:1]) for key, _, _ in groups])
        per_rung = [[dict() for _ in RUNGS] for _ in fams]
        V64 = self.V.astype(np.float64)
        A, e = self.donor_A[self.pool], self.donor_e[self.pool]
        keys = [key for key, _, _ in groups]
        D = np.stack([d for _, d, _ in groups])                                              # [G, M, 3] float32
        D64 = D.astype(np.float64)
        clamped = np.array([c for _, _, c in groups])
        G, M = D.shape[:2]
        g_ix = np.arange(G)[:, None, None, None]
        for pn, (i, j) in enumerate(pairs):
            pi, pj = upal[i], upal[j]
            n = pi - pj
            mid = (pi + pj) / 2
            # B': of the 11 reachable values nearest the midpoint per axis, the 125 points nearest the bisector plane
            vi = self.b_candidates(mid, n)
            Bc = V64[vi]
            base = 2 * (Bc - mid) @ n
            d0 = ((Bc - pi) ** 2).sum(1)
            want = centres[None, :] * d0[:, None] - base[:, None]                            # the 2 * d . n that gives each rung
            T = 2 * (D64 @ n)                                                                # [G, M]
            order = np.argsort(T, 1, kind="stable")
            T = np.take_along_axis(T, order, 1)
            pos = np.stack([np.searchsorted(T[g], want) for g in range(G)])                  # [G, 125, C]
            m = order[g_ix, np.clip(np.stack([pos - 1, pos], -1), 0, M - 1)]                 # [G, 125, C, 2]: the donors on either side
            q = self.V[vi][None, :, None, None, :] + D[g_ix, m]                              # float32
            q[clamped] = np.clip(q[clamped], F(0), F(255))
            q64 = q.astype(np.float64)
            di, dj = ((q64 - pi) ** 2).sum(-1), ((q64 - pj) ** 2).sum(-1)
            lo_d, hi_d = np.minimum(di, dj), np.maximum(di, dj)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = (hi_d - lo_d) / lo_d
            hg, hb, hc, hk = np.nonzero((lo_d > 0) & (rel <= RUNGS[-1][1]))
            if not len(hg):
                continue
            rung = rung_of(rel[hg, hb, hc, hk])
            fr = (q64[hg, hb, hc, hk] != np.floor(q64[hg, hb, hc, hk])).any(1)
            # per rung a few hits, fractional ones first; then i and j must be the two nearest colours of the whole palette
            code = fam_of[hg] * len(RUNGS) + rung
            take = np.concatenate([np.flatnonzero(code == c)[np.argsort(~fr[code == c], kind="stable")][:6] for c in np.unique(code)])
            hg, hb, hc, hk, rung, fr = hg[take], hb[take], hc[take], hk[take], rung[take], fr[take]
            qh = q64[hg, hb, hc, hk]
            dall = ((qh[:, None, :] - upal[None, :, :]) ** 2).sum(-1)
            two = np.sort(dall, 1)[:, :2]
            top = (two[:, 0] == lo_d[hg, hb, hc, hk]) & (two[:, 1] == hi_d[hg, hb, hc, hk])
            if Ku > 2:
                top &= np.partition(dall, 2, 1)[:, 2] > two[:, 1]
            for h in np.flatnonzero(top):
                per_rung[fam_of[hg[h]]][rung[h]].setdefault(pn, []).append((keys[hg[h]], int(m[hg[h], hb[h], hc[h], hk[h]]), vi[hb[h]], bool(fr[h])))
        for fam, rungs in zip(fams, per_rung):
            for r, by_pair in enumerate(rungs):
                if r == 0 and self.gamma:
                    continue          # the exact-tie rung is asked of integer palettes only
                kept = sorted(by_pair)[:PAIRS_KEPT]
                for pn in kept:
                    distinct = list({(h[0], h[1], tuple(h[2])): h for h in by_pair[pn]}.values())
                    hits = sorted(distinct, key=lambda h: not h[3])[:3]             # fractional queries first
                    for key, m, v, _ in hits:
                        found[key].append((m, v, r, pn))
                    if fam == ("pair",):
                        # (a rung is counted from the oracle's report in the CPU tier; this is the generator's own tally)
                        stats["queries"][r] += len(hits)
                        stats["fractional"][r] += sum(h[3] for h in hits)
                if fam == ("pair",):
                    stats["pairs"][r] = len(kept)
        out = {}
        for key, lst in found.items():
            if not lst:
                continue
            m = np.array([x[0] for x in lst])
            v = np.stack([x[1] for x in lst])
            out[key] = dict(A=A[m], e=e[m], B=self.rep[v], kind=np.full(len(m), K_LADDER, np.uint8),
                            rung=np.array([x[2] for x in lst], np.int8), pair=np.array([x[3] for x in lst], np.int32))
        return out

    # -------------------------------------------------------------------------------------------------- targets
    def leaves(self):
        rs = np.random.RandomState(11)
        around = (np.clip(self.pal[rs.randint(0, self.K, LEAVES // 2)] + rs.randint(-3, 4, (LEAVES // 2, 3)), 0, 255)).astype(np.int64) // 2
        return np.unique(np.concatenate([around, rs.randint(0, 128, (LEAVES, 3))]), axis=0)

    def _targets(self):
        A, e = self.donor_A[self.pool], self.donor_e[self.pool]
        cells16 = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
        leaves = self.leaves()
        groups = [(("pair", k), self.push_pair(e, w), True) for k, w in enumerate(PAIR_WEIGHTS)]
        groups += [(("tile", s), self.push_pair(e, F(w)), False) for s, w in enumerate(TILE_WEIGHTS)]
        # (the perceptual diffuser's weight follows the donor's luminance and the hybrid one's push is a linear map of the error: a
        # far finer set of pushes than sixteen powers of two, for the ladder alone)
        ladder = self._ladder(groups + [(("pair1", 1), self.push_model1(A, e), False), (("pair1", 2), self.push_model2(e), False)])
        self.pair1_ladder = {m: ladder.get(("pair1", m)) for m in (1, 2)}
        fA, fe = self.donor_A[self.far], self.donor_e[self.far]
        gA, ge = np.concatenate([A, fA]), np.concatenate([e, fe])
        for key, d, clamp in groups:
            # the cell solvers want few donors, each with a fraction on every axis and a push of less than 12: from the small errors
            # and, for the small weights, the far ones (under use_gamma the reachable B' lie up to 3 apart at the bright end, and a
            # palette whose errors all have one sign has nothing else to bridge that with)
            w = F(TILE_WEIGHTS[key[1]]) if key[0] == "tile" else PAIR_WEIGHTS[key[1]]
            gd = self.push_pair(ge, w)
            fr = np.flatnonzero((gd != np.floor(gd)).all(1) & (np.abs(gd).max(1) < 12))
            if len(fr) < 8:
                fr = np.flatnonzero((gd != np.floor(gd)).any(1))
            fr = fr[np.argsort(np.abs(gd[fr]).max(1), kind="stable")]
            sel = fr[np.linspace(0, len(fr) - 1, min(len(fr), 48)).astype(np.int64)]
            parts = [self._solve_cells(gA[sel], ge[sel], gd[sel], 16, cells16, clamp, K_GAP16),
                     self._solve_cells(gA[sel], ge[sel], gd[sel], 2, leaves, clamp, K_GAP2)]
            if clamp:
                parts.append(self._solve_face(A, e, d))
            else:
                parts.append(self._solve_out(fA, fe, self.push_pair(fe, F(TILE_WEIGHTS[key[1]]))))
            parts.append(ladder.get(key))
            self.rows[key] = _concat([p for p in parts if p is not None])

    # -------------------------------------------------------------------------------------------------- layouts
    def pair_frame(self, k, serpentine=False, rows=None):
        """the rows of weight PAIR_WEIGHTS[k] as one [R, 2, 3] frame (R even), the receiver's x per row, and the predicted
        queries [R, 2, 3].  rows: take these row numbers (cyclic filling of a launch shape) instead of all"""
        r = self.rows[("pair", k)]
        R = len(r["A"]) + (len(r["A"]) & 1)
        sel = np.arange(R) % len(r["A"]) if rows is None else np.asarray(rows) % len(r["A"])
        A, B, e = r["A"][sel], r["B"][sel], r["e"][sel]
        n = len(sel)
        rx = np.ones(n, np.int64)
        if serpentine:
            rx[1::2] = 0
        frame = np.empty((n, 2, 3), np.uint8)
        frame[np.arange(n), rx] = B
        frame[np.arange(n), 1 - rx] = A
        q = np.empty((n, 2, 3), F)
        q[np.arange(n), 1 - rx] = self.src(A)
        q[np.arange(n), rx] = np.clip(self.src(B) + self.push_pair(e, PAIR_WEIGHTS[k]), F(0), F(255))
        return frame, rx, q, sel

    def tiles(self):
        """all tile targets: (A, B, e, slot, kind, rung, pair) with `slot` the receiver that is the target"""
        parts = []
        for s in range(4):
            r = dict(self.rows[("tile", s)])
            r["slot"] = np.full(len(r["A"]), s, np.uint8)
            parts.append(r)
        return _concat(parts)

    def tile_frames(self, n, h, w, banded=False):
        """frames [n, h, w, 3], gate [n, h, w], predicted queries [n, h, w, 3] and a target map [n, h, w] (index into tiles(), -1
        elsewhere) with the tile targets dealt cyclically over the n * (h // 2) * (w // 3) tiles.  banded: the tiles are ordered so
        that the first 64-row bands hold inside targets only, the last ones tiles whose target is outside, and the band between
        exactly one outside receiver."""
        t = self.tiles()
        T = len(t["A"])
        th, tw = h // 2, w // 3
        slots = n * th * tw
        order = np.arange(T)
        d_t = self.push_pair(t["e"], np.array(TILE_WEIGHTS, F)[t["slot"]][:, None])
        q_t = self.src(t["B"]) + d_t
        outside = ((q_t < 0) | (q_t > 255)).any(1)
        if banded:
            order = self._banded(t, tw)
            assert len(order) <= slots, "the frame is too small for the banded order: take tile_spread_shape()"
            order = np.concatenate([order, order[-(32 * tw):][np.arange(slots - len(order)) % (32 * tw)]])
        sel = order[np.arange(slots) % len(order)].reshape(n, th, tw)
        frame = np.zeros((n, h, w, 3), np.uint8)
        frame[...] = self.rep[len(self.rep) // 2]
        gate = np.zeros((n, h, w), np.uint8)
        tmap = np.full((n, h, w), -1, np.int64)
        A, B, e = t["A"][sel], t["B"][sel], t["e"][sel]
        H2, W3 = th * 2, tw * 3
        frame[:, 0:H2:2, 1:W3:3] = A
        gate[:, 0:H2:2, 1:W3:3] = 1
        q = self.src(frame)
        for s, (dy, dx) in enumerate(TILE_SLOTS):
            frame[:, dy:H2:2, dx:W3:3] = B
            q[:, dy:H2:2, dx:W3:3] = self.src(B) + self.push_pair(e, F(TILE_WEIGHTS[s]))
            tmap[:, dy:H2:2, dx:W3:3] = np.where(t["slot"][sel] == s, sel, -1)
        return frame, gate, q, tmap

    def _banded(self, t, tw):
        """the tile targets in whole 64-row bands of tw tiles a row: bands of tiles none of whose four receivers is outside the
        cube, one such band with a single tile that has exactly one receiver outside, the tiles with several, and a last band of
        tiles whose target is outside"""
        per_band = 32 * tw
        q4 = self.src(t["B"])[:, None, :] + self.push_pair(t["e"][:, None, :], np.array(TILE_WEIGHTS, F)[None, :, None])
        out4 = ((q4 < 0) | (q4 > 255)).any(2)
        n_out = out4.sum(1)
        target_out = out4[np.arange(len(n_out)), t["slot"]]
        clean, one, rest, dirty = np.flatnonzero(n_out == 0), np.flatnonzero(n_out == 1), np.flatnonzero(n_out > 0), np.flatnonzero(target_out)

        def whole(ix, fill):
            """ix, filled up to whole bands from `fill`"""
            pad = -len(ix) % per_band
            return np.concatenate([ix, fill[np.arange(pad) % len(fill)]]) if pad else ix
        parts = [whole(clean, clean)]
        if len(one):
            band = clean[np.arange(per_band) % len(clean)].copy()
            band[per_band // 2] = one[0]
            parts.append(band)
        if len(rest):
            parts.append(whole(rest, dirty if len(dirty) else rest))
        if len(dirty):
            parts.append(dirty[np.arange(per_band) % len(dirty)])
        return np.concatenate(parts)

    def tile_spread_shape(self, w=825):
        """(1, h, w) of the one frame that holds tile_frames(banded=True): at least four bands, w >= 64"""
        bands = len(self._banded(self.tiles(), w // 3)) // (32 * (w // 3))
        return 1, 64 * max(bands, 4), w

    def pair1_frames(self, model, n):
        """frames [n, 1, 2, 3] for the perceptual (1) / hybrid (2) diffuser and the predicted queries: `out` targets for this
        model's own push, then donors and receivers drawn at random"""
        fA, fe = self.far_A, self.far_e
        d = self.push_model1(fA, fe) if model == 1 else self.push_model2(fe)
        r = self._solve_out(fA, fe, d)
        rs = np.random.RandomState(model)
        m = rs.randint(0, len(fA), n)
        A, e = fA[m], fe[m]
        B = rs.randint(0, 256, (n, 3)).astype(np.uint8)
        r = _concat([p for p in (self.pair1_ladder[model], r) if p is not None]) if (r is not None or self.pair1_ladder[model] is not None) else None
        kind = np.zeros(n, np.uint8)
        rung = np.full(n, -1, np.int8)
        if r is not None:
            k = min(n, len(r["A"]))
            A[:k], e[:k], B[:k], kind[:k], rung[:k] = r["A"][:k], r["e"][:k], r["B"][:k], r["kind"][:k], r["rung"][:k]
        self.pair1_kind = {**getattr(self, "pair1_kind", {}), model: (kind, rung)}
        frame = np.stack([A, B], 1)[:, None]
        push = self.push_model1(A, e) if model == 1 else self.push_model2(e)
        q = np.stack([self.src(A), self.src(B) + push], 1)[:, None]
        return np.ascontiguousarray(frame), q

    def describe(self, q, key=None, row=None):
        """a query point for a failure message: the point, its 16^3 cell, and what kind of target it is"""
        c = np.clip(np.floor(q), 0, 255).astype(int) >> 4
        s = f"query ({float(q[0])!r}, {float(q[1])!r}, {float(q[2])!r}) cell ({c[0]},{c[1]},{c[2]})"
        if key is not None and row is not None:
            r = self.rows[key]
            s += f" {KINDS[r['kind'][row]]}"
            if r["kind"][row] == K_LADDER:
                s += f" rung {RUNG_NAMES[r['rung'][row]]}"
        return s


def _concat(parts):
    n = [len(p["A"]) for p in parts]
    out = {}
    for k in ("A", "B", "e", "kind"):
        out[k] = np.concatenate([p[k] for p in parts])
    for k, fill, dt in (("rung", -1, np.int8), ("pair", -1, np.int32), ("slot", 0, np.uint8)):
        if any(k in p for p in parts):
            out[k] = np.concatenate([p[k] if k in p else np.full(c, fill, dt) for p, c in zip(parts, n)])
    if "rung" not in out:
        out["rung"] = np.full(sum(n), -1, np.int8)
        out["pair"] = np.full(sum(n), -1, np.int32)
    return out


_STEER = {}


def steer(orc, name, gamma):
    key = (name, bool(gamma))
    if key not in _STEER:
        _STEER[key] = Steer(orc, name, gamma)
    return _STEER[key]


def release():
    _STEER.clear()
    _cube.cache_clear()


# ------------------------------------------------------------------------------------------------------ classification
def rel_gap(pal_f32, q):
    """(d1 - d0) / d0 of the float64 squared distances from q [n, 3] to the two nearest DISTINCT colours, and their numbers in
    np.unique(pal, axis=0)"""
    upal = np.unique(pal_f32.astype(np.float64), axis=0)
    q = q.astype(np.float64)
    d = ((q[:, None, :] - upal[None, :, :]) ** 2).sum(-1)
    two = np.argsort(d, 1, kind="stable")[:, :2]
    d0, d1 = np.take_along_axis(d, two, 1).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d0 > 0, (d1 - d0) / d0, np.inf), np.sort(two, 1)


def rung_of(rel):
    r = np.full(len(rel), -1, np.int64)
    r[rel == 0] = 0
    for k in range(1, len(RUNGS)):
        r[(rel > RUNGS[k][0]) & (rel <= RUNGS[k][1])] = k
    return r


def direction_of(q):
    """-1 / 0 / +1 per axis: below 0, inside [0, 255], above 255"""
    return (q > 255).astype(np.int64) - (q < 0).astype(np.int64)


# Axes on which a palette has no colour BELOW its nearest entry: no error is negative there, so no push goes that way, nothing
# overshoots the face at 0 and no query lies beyond it.  `two` = [(0,0,0), (2,0,0)]: g and b of every colour are >= the
# entries' 0; on r the colour 1 is a tie that the tree gives to (0,0,0), and under use_gamma the entries are 0 and 0.155
# with the linear values integers.  Every other palette has errors of both signs on every axis.
NO_NEGATIVE_ERROR = {("two", False): (0, 1, 2), ("two", True): (0, 1, 2)}


def unreachable_directions(name, gamma):
    """the directions of DIRECTIONS no push of this palette's errors points in"""
    axes = NO_NEGATIVE_ERROR.get((name, bool(gamma)), ())
    return {d for d in DIRECTIONS if any(d[a] < 0 for a in axes)}


def beyond(q):
    """how far a query is beyond the cube (0 inside): the largest overshoot of a coordinate"""
    return np.maximum(np.maximum(-q, q - 255), 0).max(-1)


# ------------------------------------------------------------------------------------------------------ saturate
def bright_palette(orc):
    """mc256 mirrored: a palette near white, for the black frame"""
    return [tuple(255 - v for v in c) for c in cr.palette(orc, "mc256")]


def saturate_frames(h, w):
    """{name: frame [h, w, 3]}: flat frames far from a dark (or, black: a bright) palette, and a ramp through both ends"""
    y, x = np.mgrid[0:h, 0:w]
    flat = {"white": (255, 255, 255), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255), "yellow": (255, 255, 0), "black": (0, 0, 0)}
    out = {k: np.broadcast_to(np.array(v, np.uint8), (h, w, 3)).copy() for k, v in flat.items()}
    out["ramp"] = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), 255 - (x * 255) // max(w - 1, 1)], -1).astype(np.uint8)
    return out


# WALL seconds of Steer(...) per palette (integer, use_gamma), dictionary and targets together, as printed by
# tests/test_steer_cpu.py::test_generator_cost on 8 cores:
GENERATOR_SECONDS = {"two": (15.5, 8.8), "palr16": (11.3, 11.2), "mc64": (17.3, 12.1), "clustered200": (11.6, 10.7), "dup256": (10.8, 11.1),
                     "palr256": (10.0, 11.3), "palr300": (10.5, 13.1), "palr1024": (11.1, 13.7)}
