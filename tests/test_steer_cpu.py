"""CPU tier of the steered-query tests (tests/steer_ref.py): the oracle reports the points it looks up without changing a
result; the generator's predicted queries equal that report bit for bit in every layout; a donor asks about its own pixel; and
the floors of steer_ref's docstring hold -- all of it read from the oracle's report, nothing from a device.

(The mutation check the design asked for -- corrupt one candidate list of the host tables and watch a gap target fall into it --
is not here: ed_tables_build (ed_tables.h) is not reachable through the host C ABI, only from the library's own launch path.)"""
import numpy as np
import pytest

import cube_ref as cr
import steer_ref as sr

CASES = [(n, g) for n in sr.PALETTES for g in cr.GAMMAS]
IDS = [f"{n}-{'gamma' if g else 'int'}" for n, g in CASES]


@pytest.fixture(scope="module", autouse=True)
def _release():
    """the generators (and the cube) stay in memory while this module runs, not longer"""
    yield
    sr.release()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pair_dump(orc, S, k, serp):
    frame, rx, q, sel = S.pair_frame(k, serp)
    out, dump = orc.error_diffusion_u8(frame, S.pal, S.out_colors, S.lut, serpentine=serp, taps=[(1, 0, sr.PAIR_WEIGHTS[k])], div=1.0,
                                       want_queries=True)
    return frame, rx, q, sel, out, dump


# ------------------------------------------------------------------------------------------------------ the oracle's report
def test_the_report_changes_no_result(orc):
    arr = orc.rnd(37, 53, 4)
    pal_f32, out_colors, lut_in = orc.prepare_palette(orc.palr(40, 3), True)
    for serp in (False, True):
        plain = orc.error_diffusion_u8(arr, pal_f32, out_colors, lut_in, "floyd_steinberg", serp)
        taps, div = orc.ed_kernel("floyd_steinberg")
        out, q = orc.error_diffusion_u8(arr, pal_f32, out_colors, lut_in, serpentine=serp, taps=taps, div=div, want_queries=True)
        assert np.array_equal(plain, out)
        assert q.shape == arr.shape and q.dtype == np.float32 and q.min() >= 0 and q.max() <= 255      # clamped
        assert np.array_equal(q[0, 0], lut_in[arr[0, 0]].astype(np.float32))
    gate = (orc.rnd(37, 53, 5)[..., 0] > 90).astype(np.uint8)
    for model, kw in ((1, {}), (2, dict(p0=1.0, p1=0.2)), (3, dict(gate=gate)), (4, dict(serpentine=True))):
        plain = orc.var_diffusion_u8(arr, pal_f32, out_colors, lut_in, model, **kw)
        out, q = orc.var_diffusion_u8(arr, pal_f32, out_colors, lut_in, model, want_queries=True, **kw)
        assert np.array_equal(plain, out)
        assert (q.min() >= 0 and q.max() <= 255) == (model == 4), model      # only Ostromoukhov clamps; the others leave the cube here
    with pytest.raises(ValueError):
        orc.error_diffusion_u8(arr, pal_f32, out_colors, lut_in, taps=[(1, 0, 1.0)])


def test_explicit_coefficient_table(orc):
    arr = orc.rnd(20, 31, 6)
    pal_f32, out_colors, lut_in = orc.prepare_palette(orc.palr(16, 3), False)
    own = orc.var_diffusion_u8(arr, pal_f32, out_colors, lut_in, 4)
    assert np.array_equal(own, orc.var_diffusion_u8(arr, pal_f32, out_colors, lut_in, 4, coef=orc.ostromoukhov_coefficients()))
    assert not np.array_equal(own, orc.var_diffusion_u8(arr, pal_f32, out_colors, lut_in, 4, coef=np.zeros((256, 3), np.float32)))


# ------------------------------------------------------------------------------------------------------ floors
def _gap_floor(q, width, cells, clamped, what):
    """q: the reported queries of the receivers [n, 3]"""
    ip = np.floor(q)
    frac = q != ip
    q = q[frac.any(1)]
    ip, frac = np.floor(q), q != np.floor(q)
    inside = ((q >= 0) & (q < 256)).all(1)
    q, ip, frac = q[inside], ip[inside].astype(np.int64), frac[inside]
    c = ip // width
    nc = 256 // width
    lin = (c[:, 0] * nc + c[:, 1]) * nc + c[:, 2]
    want = (cells[:, 0] * nc + cells[:, 1]) * nc + cells[:, 2]
    count = np.bincount(lin, minlength=nc ** 3)[want]
    assert (count >= 8).all(), f"{what}: {int((count < 8).sum())} of {len(cells)} cells of width {width} get fewer than 8 fractional queries, e.g. {cells[count < 8][:4].tolist()}"
    last = c * width + width - 1
    if clamped:
        last = np.minimum(last, 254)
    for a in range(3):
        on = (ip[:, a] == last[:, a]) & frac[:, a]
        have = np.bincount(lin[on], minlength=nc ** 3)[want] > 0
        assert have.all(), f"{what}: axis {a}: {int((~have).sum())} cells of width {width} have no query on their last integer part, e.g. {cells[~have][:4].tolist()}"


@pytest.mark.parametrize("name,gamma", CASES, ids=IDS)
def test_pair_layout(orc, name, gamma):
    """prediction == report for all sixteen weights and both scans; a donor asks about its own pixel; gap, face and ladder floors"""
    S = sr.steer(orc, name, gamma)
    cells16 = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    recv, lad_q, raw = [], [], []
    for k in range(len(sr.PAIR_WEIGHTS)):
        for serp in (False, True):
            frame, rx, q, sel, out, dump = _pair_dump(orc, S, k, serp)
            n = np.arange(len(rx))
            assert np.array_equal(_bits(q), _bits(dump)), f"weight 2^-{k + 1} serpentine={serp}: predicted queries differ from the oracle's"
            assert np.array_equal(dump[n, 1 - rx], S.src(frame[n, 1 - rx]))          # isolation: nothing reaches a donor
            if not serp:
                recv.append(dump[n, rx])
                # (what the receiver held before the clamp; clamped, it is the prediction that was just compared)
                raw.append(S.src(frame[n, rx]) + S.push_pair(S.rows[("pair", k)]["e"][sel], sr.PAIR_WEIGHTS[k]))
                lad = S.rows[("pair", k)]["kind"][sel] == sr.K_LADDER
                lad_q.append(dump[n, rx][lad])
        # Ostromoukhov with rows {w, 0, 0} asks the same questions
        frame, rx, q, sel = S.pair_frame(k, False)
        coef = np.zeros((256, 3), np.float32)
        coef[:, 0] = sr.PAIR_WEIGHTS[k]
        _, dump = orc.var_diffusion_u8(frame, S.pal, S.out_colors, S.lut, 4, coef=coef, want_queries=True)
        assert np.array_equal(_bits(q), _bits(dump)), f"Ostromoukhov, weight 2^-{k + 1}"
    recv = np.concatenate(recv)
    _gap_floor(recv, 16, cells16, True, f"{name} pair")
    _gap_floor(recv, 2, S.leaves(), True, f"{name} pair")
    assert len(S.leaves()) >= sr.LEAVES
    # face: all 26 faces, edges and corners, the free coordinates fractional
    on_lo, on_hi = recv == 0, recv == 255
    free_frac = (recv != np.floor(recv)) | on_lo | on_hi
    sig = (on_hi.astype(np.int64) - on_lo.astype(np.int64))[free_frac.all(1)]
    seen = {tuple(s) for s in np.unique(sig, axis=0).tolist()}
    assert set(sr.DIRECTIONS) <= seen, f"faces without a query: {sorted(set(sr.DIRECTIONS) - seen)}"
    # ... and by OVERSHOOT in every direction the palette's errors point in: the value before the clamp lies beyond the face
    raw = np.concatenate(raw)
    assert np.array_equal(np.clip(raw, 0, 255), recv)
    over = sr.direction_of(raw)[free_frac.all(1)]
    by_overshoot = {tuple(x) for x in np.unique(over, axis=0).tolist()} - {(0, 0, 0)}
    assert by_overshoot == set(sr.DIRECTIONS) - sr.unreachable_directions(name, gamma), sorted(set(sr.DIRECTIONS) - by_overshoot)
    _ladder_floor(S, np.concatenate(lad_q), f"{name} gamma={gamma} pair")


def ladder_counts(S, q):
    """per rung: (queries, distinct colour pairs, fractional queries) among the reported queries q"""
    rel, pairs = sr.rel_gap(S.pal, q) if len(q) else (np.zeros(0), np.zeros((0, 2), np.int64))
    rung = sr.rung_of(rel)
    frac = (q != np.floor(q)).any(1) if len(q) else np.zeros(0, bool)
    return [(int((rung == r).sum()), len(np.unique(pairs[rung == r], axis=0)) if (rung == r).any() else 0, int(frac[rung == r].sum()))
            for r in range(len(sr.RUNGS))]


def _ladder_floor(S, q, what, layout="pair"):
    """The floor of every rung from the oracle's report, or -- where the layout's pushes cannot reach a rung for this palette --
    exactly the count recorded in steer_ref.LADDER_RECORDED[layout, palette, use_gamma]."""
    st = S.ladder_stats
    print(f"{what}: {st['adjacent']} adjacent pairs, floor {st['floor']}")
    recorded = sr.LADDER_RECORDED.get((layout, S.name, S.gamma), {})
    for r, (n_q, n_pairs, n_frac) in enumerate(ladder_counts(S, q)):
        if r == 0 and S.gamma:
            continue
        print(f"  rung {sr.RUNG_NAMES[r]}: {n_q} queries from {n_pairs} pairs, {n_frac} fractional")
        if r in recorded:
            assert n_pairs == recorded[r] < st["floor"], f"{what}: rung {sr.RUNG_NAMES[r]}: {n_pairs} pairs, recorded {recorded[r]}"
        else:
            assert n_pairs >= st["floor"], f"{what}: rung {sr.RUNG_NAMES[r]}: {n_pairs} pairs, floor {st['floor']}"
        few = sr.TIE_FRACTIONAL_RECORDED.get((layout, S.name, S.gamma)) if r == 0 else None
        if few is not None:
            assert n_frac == few and 2 * few < n_q, f"{what}: exact ties: {n_frac} of {n_q} fractional, recorded {few}"
        elif n_pairs:
            assert 2 * n_frac >= n_q, f"{what}: rung {sr.RUNG_NAMES[r]}: fewer than half of the queries are fractional"


@pytest.mark.parametrize("name,gamma", CASES, ids=IDS)
def test_tile_layout(orc, name, gamma):
    """adaptive variance with the gate on the donors only: prediction == report (so nothing reaches a donor or an idle pixel);
    gap floors; queries beyond the cube in every direction the palette's errors reach; the three kinds of 64-row bands"""
    S = sr.steer(orc, name, gamma)
    n, h, w = S.tile_spread_shape()
    frame, gate, q, tmap = S.tile_frames(n, h, w, banded=True)
    assert len(np.unique(tmap[tmap >= 0])) == len(S.tiles()["A"]), "the frame does not hold every tile target"
    _, dump = orc.var_diffusion_u8(frame[0], S.pal, S.out_colors, S.lut, 3, gate=gate[0], want_queries=True)
    assert np.array_equal(_bits(q[0]), _bits(dump)), "predicted queries differ from the oracle's"
    idle = np.ones((h, w), bool)
    for dy, dx in sr.TILE_SLOTS:
        idle[dy:(h // 2) * 2:2, dx:(w // 3) * 3:3] = False
    assert np.array_equal(dump[idle], S.src(frame[0][idle]))
    recv = dump[tmap[0] >= 0]
    cells16 = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    _gap_floor(recv, 16, cells16, False, f"{name} tile")
    _gap_floor(recv, 2, S.leaves(), False, f"{name} tile")
    # beyond the cube: every direction the palette's errors point in, and in it every distance class that some donor's push reaches
    # with the largest weight: near 1, 16 and 64 means within [lo, 2 lo), the last class at least 100
    e = S.far_e
    dist = sr.beyond(recv)
    dirs = sr.direction_of(recv)
    far = 0
    for d in sr.DIRECTIONS:
        dd = np.array(d, np.float32)
        reach = np.where(dd != 0, e * dd * np.float32(7.0 / 16), np.inf).min(1).max()
        mine = (dirs == np.array(d)).all(1)
        assert (reach > 0) == (d not in sr.unreachable_directions(S.name, S.gamma)), (d, reach)
        for lo in sr.OUT_DISTANCES:
            if reach >= lo:
                hi = np.inf if lo == sr.OUT_DISTANCES[-1] else 2 * lo
                assert (mine & (dist >= lo) & (dist < hi)).any(), f"direction {d}: no query {lo} beyond the cube although a push reaches {reach}"
                far = max(far, lo)
    seen = {tuple(x) for x in np.unique(dirs, axis=0).tolist()} - {(0, 0, 0)}
    assert seen == set(sr.DIRECTIONS) - sr.unreachable_directions(S.name, S.gamma), sorted(set(sr.DIRECTIONS) - seen)
    print(f"{name} gamma={gamma} tile: furthest query {dist.max():.1f} beyond the cube, distance classes up to {far}")
    # bands of 64 rows: inside only / exactly one outside pixel / every target receiver outside
    out_px = ((dump < 0) | (dump > 255)).any(-1)
    per_band = out_px.reshape(h // 64, 64, w).sum((1, 2))
    assert (per_band == 0).any() and (per_band == 1).any()
    tgt_out = (out_px & (tmap[0] >= 0)).reshape(h // 64, 64, w).sum((1, 2)) == (tmap[0] >= 0).reshape(h // 64, 64, w).sum((1, 2))
    assert tgt_out.any(), "no band whose target receivers are all outside"
    lad = S.tiles()["kind"][np.maximum(tmap[0], 0)] == sr.K_LADDER
    lad_q = dump[(tmap[0] >= 0) & lad]
    _ladder_floor(S, lad_q, f"{name} gamma={gamma} tile", "tile")


@pytest.mark.parametrize("model", (1, 2))
@pytest.mark.parametrize("name,gamma", sr.PAIR1_CASES, ids=[f"{n}-{'gamma' if g else 'int'}" for n, g in sr.PAIR1_CASES])
def test_pair1_layout(orc, name, gamma, model):
    """the very frames the GPU tier launches (steer_ref.PAIR1_CASES, PAIR1_FRAMES): prediction == report, queries beyond the cube, and
    the ladder's floors for this diffuser's own pushes"""
    S = sr.steer(orc, name, gamma)
    frames, q = S.pair1_frames(model, sr.PAIR1_FRAMES)
    kw = dict(p0=1.0, p1=0.2) if model == 2 else {}
    dump = np.stack([orc.var_diffusion_u8(f, S.pal, S.out_colors, S.lut, model, want_queries=True, **kw)[1] for f in frames])
    assert np.array_equal(_bits(q), _bits(dump))
    assert np.array_equal(dump[:, 0, 0], S.src(frames[:, 0, 0]))
    assert sr.beyond(dump[:, 0, 1]).max() > 0
    kind, _ = S.pair1_kind[model]
    _ladder_floor(S, dump[:, 0, 1][kind == sr.K_LADDER], f"{name} gamma={gamma} model {model} pair1", f"pair1-{model}")


@pytest.mark.parametrize("gamma", cr.GAMMAS, ids=["int", "gamma"])
def test_two_recorded_zeros_are_exhaustive(orc, gamma):
    """`two` has ONE adjacent pair, so the ladder's whole search space -- every donor of the pool, the 125 B', every weight of every
    layout -- can be enumerated: no query of it lies on a rung that LADDER_RECORDED gives as 0 (the search proper looks only at the
    two donors on either side of each rung's centre)."""
    S = sr.steer(orc, "two", gamma)
    upal = np.unique(S.pal.astype(np.float64), axis=0)
    assert len(upal) == 2
    vi = S.b_candidates((upal[0] + upal[1]) / 2, upal[0] - upal[1])
    Bq = S.V[vi]
    A, e = S.pool_A, S.pool_e
    groups = [("pair", S.push_pair(e, w), True) for w in sr.PAIR_WEIGHTS] + [("tile", S.push_pair(e, np.float32(w)), False) for w in sr.TILE_WEIGHTS]
    if ("two", gamma) in sr.PAIR1_CASES:
        groups += [("pair1-1", S.push_model1(A, e), False), ("pair1-2", S.push_model2(e), False)]
    seen = {}
    for layout, d, clamp in groups:
        q = (Bq[:, None, :] + d[None, :, :]).reshape(-1, 3)
        if clamp:
            q = np.clip(q, 0, 255)
        rung = sr.rung_of(sr.rel_gap(S.pal, q)[0])
        seen.setdefault(layout, set()).update(np.unique(rung[rung >= 0]).tolist())
    for layout, rungs in seen.items():
        zero = {r for r, c in sr.LADDER_RECORDED.get((layout, "two", gamma), {}).items() if c == 0}
        print(f"two gamma={gamma} {layout}: the space holds queries on rungs {sorted(rungs)}, recorded as empty {sorted(zero)}")
        assert not (rungs & zero), (layout, sorted(rungs & zero))


def test_saturated_frames_leave_the_cube_far_behind(orc):
    """the oracle's report measures what the saturate layout is for: queries hundreds to thousands of units beyond the cube"""
    for pal_name, frames in (("mc256", ("white", "red", "green", "blue", "yellow", "ramp")), ("bright", ("black",)), ("palr16", ("white", "black"))):
        pal = sr.bright_palette(orc) if pal_name == "bright" else cr.palette(orc, pal_name)
        pal_f32, _, lut_in = orc.prepare_palette(pal, False)
        oc = cr.index_colours(len(pal_f32))
        furthest = {}
        for fname in frames:
            frame = sr.saturate_frames(64, 96)[fname]
            for model, kw in ((1, {}), (2, dict(p0=1.0, p1=0.2)), (3, dict(gate=np.ones((64, 96), np.uint8)))):
                _, q = orc.var_diffusion_u8(frame, pal_f32, oc, lut_in, model, want_queries=True, **kw)
                far = sr.beyond(q).max()
                print(f"{pal_name} {fname} model {model}: furthest query {far:.0f} beyond the cube")
                # every frame goes beyond the outermost 16-wide ring of cells
                if fname != "ramp":
                    assert far >= 16, (pal_name, fname, model, far)
                furthest[model] = max(furthest.get(model, 0), far)
        # the adaptive diffuser pushes the whole error on, which grows with the frame: thousands; the perceptual one scales it by the
        # luminance (a half on black) and the hybrid one keeps a fifth of the colour part, so they level off: hundreds
        assert furthest[3] >= 1000 and furthest[1] >= 100 and furthest[2] >= 100, (pal_name, furthest)


def test_generator_cost(orc):
    """wall seconds per palette, as recorded in steer_ref.GENERATOR_SECONDS (printed; the bound is the ~10 s aimed at with slack for a
    loaded machine)"""
    for name, gamma in CASES:
        S = sr.steer(orc, name, gamma)
        print(f"{name} gamma={gamma}: {S.seconds:.1f} s, {S.n_donors} donors, "
              f"{sum(len(r['A']) for k, r in S.rows.items() if k[0] == 'pair')} pair rows, {len(S.tiles()['A'])} tiles")
        assert S.seconds < 120
