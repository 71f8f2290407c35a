"""CPU tier of the ordered dither's kernel choice (dither_pie_amd/csrc/ordered_plan.h: plan_ordered, what launch_ordered asks
before it launches).  The stand-alone host_asan build prints the plan of every case (`orderedplan`), and every printed field
must equal what tests/ordered_plan_ref.py -- a transcription of the launcher as it was before the planner existed -- says:
over a grid of palette tables, thresholds, modes and the five experiment switches, and on named rows at each LDS budget
exactly and one step over.  The grid must reach every kernel instantiation the launcher's lookup names (KERNELS), no other."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import ordered_plan_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
MODES = (ref.NEAREST, ref.MATRIX, ref.IGN)

# (family, MODE, BW, ADAPT, WARP, HALF) of every pass-1 kernel that tile_kernel / brute_kernel (ordered.hip) can name; the
# brute family stands for ordered_int_kernel and ordered_f64_kernel alike
KERNELS = (
    {("brute", m, 8, 0, 0, 0) for m in (0, 1, 2, 3)} |
    {("cell", m, 8, 0, 0, 0) for m in (0, 1, 2, 3)} |
    {("fast", m, bw, 0, 0, 0) for m in (0, 1, 2, 3) for bw in (4, 8)} |
    {("lean", m, bw, ad, wp, hf) for m in (0, 1, 2, 3)
     for bw, ad, wp, hf in ((4, 0, 1, 0), (8, 1, 1, 0), (8, 0, 1, 0), (4, 0, 0, 1), (4, 0, 0, 0), (8, 1, 0, 0), (8, 0, 0, 0))} |
    {("compact", m, 8, 0, wp, hf) for m in (0, 1, 2, 3) for wp in (0, 1) for hf in (0, 1)} |
    {("lean_float", m, 8, 0, 0, 0) for m in (0, 2, 3)} |
    {("compact_float", m, 8, 0, 0, 0) for m in (0, 2, 3)})
FAMILIES = {"brute", "cell", "fast", "lean", "compact", "lean_float", "compact_float"}

BASE = dict(mode=ref.NEAREST, K=256, is_integer=1, n_inner=51, n_px=3 * 120 * 203, hw=120 * 203, w=203, y0=0, x0=0, aligned=1,
            cell_tab=0, tab_words=0, tab_total=0, cell_tab4=0, tab4_words=0, warp_tab=0, warp_words=0, warp_total=0, warp_bw=0,
            warp_adapt=0, adapt=0, cell_perm=0, cell_perm4=0, n_wide=0, n_wide4=0, comp_tab=0, comp_words=0, comp_warp=0,
            ftab=0, ftab_words=0, m=0, mpad=0, fpad=0, th_h=1, th_w=1, tw_pad=0,
            n_cus=8)    # 18 tiles on 8 CUs: one and two workgroups per CU give different grids and tile strides
NO_SWITCH = dict.fromkeys(ref.SWITCH_FIELDS, 0)

PLAIN8 = dict(cell_tab=1, tab_words=4096 * 8, tab_total=4096 * 8)
TABLES = {
    "none": {},
    "plain8_whole": PLAIN8,
    "plain8_partly_staged": dict(PLAIN8, tab_total=4096 * 8 + 512),
    "plain8_over_lean_budget": dict(cell_tab=1, tab_words=39000, tab_total=39000),
    "plain4_half": dict(PLAIN8, cell_tab4=1, tab4_words=4096 * 4),
    "plain4_over_half": dict(PLAIN8, cell_tab4=1, tab4_words=19000),
    "warped4": dict(PLAIN8, warp_tab=1, warp_bw=4, warp_words=4096 * 4 + 256, warp_total=4096 * 4 + 256),
    "warped8": dict(PLAIN8, warp_tab=1, warp_bw=8, warp_words=33000, warp_total=33400),
    "warped8_adapt": dict(PLAIN8, warp_tab=1, warp_bw=8, warp_words=33000, warp_total=33400, warp_adapt=1),
}
COMPACT = {"none": {}, "half": dict(comp_tab=1, comp_words=(4096 + 8 * 100) * 2), "full": dict(comp_tab=1, comp_words=30000),
           "too_large": dict(comp_tab=1, comp_words=41000)}
BAYER8 = dict(m=1, mpad=1, fpad=1, th_h=8, th_w=8, tw_pad=11)
THRESHOLDS = {"none": {}, "integer": BAYER8, "integer_over_256": dict(m=1, mpad=1, fpad=1, th_h=32, th_w=32, tw_pad=35),
              "float": dict(fpad=1, th_h=32, th_w=32, tw_pad=35), "neither": dict(th_h=600, th_w=600)}


def _grid():
    switch_sets = [dict(zip(ref.SWITCH_FIELDS, bits)) for bits in itertools.product((0, 1), repeat=len(ref.SWITCH_FIELDS))]
    for tab, comp, thr in itertools.product(TABLES.values(), COMPACT.values(), THRESHOLDS.values()):
        for mode, integer, aligned, adapt, perm in itertools.product(MODES, (1, 0), (1, 0), (0, 1), (0, 1)):
            f = dict(BASE, **tab, **comp, **thr, mode=mode, is_integer=integer, aligned=aligned, adapt=adapt, cell_perm=perm,
                     cell_perm4=perm, n_wide=3 * perm, n_wide4=5 * perm)
            f["comp_warp"] = f["comp_tab"] & f["warp_tab"]
            if not integer and tab:
                f.update(ftab=1, ftab_words=20000)
            for sw in switch_sets:
                yield f, sw


def _row(family, **facts):
    """A named row: the facts over BASE, and the family the parent's rules give it, worked out by hand."""
    sw = {k: facts.pop(k) for k in list(facts) if k in ref.SWITCH_FIELDS}
    return family, dict(BASE, **facts), dict(NO_SWITCH, **sw)


def _named():
    lean_words = ref.K_LEAN_TAB_BYTES // 4
    half_words = ref.K_LEAN_HALF_TAB_BYTES // 4
    bayer_words = 8 * 11
    rows = {}
    # kLeanTabBytes: the table alone, and the table with integer thresholds behind it
    rows["lean_tab_exact"] = _row("lean", cell_tab=1, tab_words=lean_words, tab_total=lean_words)
    rows["lean_tab_over"] = _row("cell", cell_tab=1, tab_words=lean_words + 1, tab_total=lean_words + 1)
    rows["lean_tab_over_partly_staged"] = _row("brute", cell_tab=1, tab_words=lean_words + 1, tab_total=lean_words + 9)
    rows["lean_thr_exact"] = _row("lean", mode=ref.MATRIX, cell_tab=1, tab_words=lean_words - bayer_words, tab_total=lean_words, **BAYER8)
    rows["lean_thr_over"] = _row("lean", mode=ref.MATRIX, cell_tab=1, tab_words=lean_words - bayer_words + 1, tab_total=lean_words, **BAYER8)
    rows["lean_thr_over_no_fpad"] = _row("brute", mode=ref.MATRIX, cell_tab=1, tab_words=lean_words - bayer_words + 1, tab_total=lean_words,
                                         **dict(BAYER8, fpad=0))
    # kLeanHalfTabBytes
    for name, extra in (("half_tab_exact", 0), ("half_tab_over", 1)):
        rows[name] = _row("lean", **PLAIN8, cell_tab4=1, tab4_words=half_words + extra)
        rows[name + "_matrix"] = _row("lean", mode=ref.MATRIX, **PLAIN8, cell_tab4=1, tab4_words=half_words - bayer_words + extra, **BAYER8)
    rows["half_tab_exact_switched_off"] = _row("lean", **PLAIN8, cell_tab4=1, tab4_words=half_words, lean_no_half=1)
    # the fast kernel: its fixed part (steps of one wide list, 64 bytes) and fixed part + integer thresholds (steps of 4 bytes)
    wide_max = (ref.LDS_BYTES - ref.fast_fixed_bytes(8, 0)) // (ref.K_WIDE_LIST * 4)
    assert ref.fast_fixed_bytes(8, wide_max) == ref.LDS_BYTES
    rows["fast_fixed_exact"] = _row("fast", **PLAIN8, cell_perm=1, n_wide=wide_max)
    rows["fast_fixed_over"] = _row("lean", **PLAIN8, cell_perm=1, n_wide=wide_max + 1)
    thr_max = (ref.LDS_BYTES - ref.fast_fixed_bytes(8, 0)) // 4
    for name, extra in (("fast_thr_exact", 0), ("fast_thr_over", 1)):
        rows[name] = _row("fast", mode=ref.MATRIX, **PLAIN8, cell_perm=1, fast_all=1, m=1, mpad=1, fpad=1, th_h=1, th_w=thr_max + extra - 3,
                          tw_pad=thr_max + extra)
    rows["fast_matrix_without_switch"] = _row("lean", mode=ref.MATRIX, **PLAIN8, cell_perm=1, **BAYER8)
    # the compact kernel: kCompactHalfWords and all of LDS
    for name, limit in (("compact_half", 4 * ref.K_COMPACT_HALF_WORDS), ("compact_full", ref.LDS_BYTES)):
        words = (limit - ref.K_COMPACT_TAB_AT) // 4
        rows[name + "_exact"] = _row("compact", **PLAIN8, adapt=1, comp_tab=1, comp_words=words)
        rows[name + "_over"] = _row("compact" if name == "compact_half" else "lean", **PLAIN8, adapt=1, comp_tab=1, comp_words=words + 1)
        rows[name + "_exact_matrix"] = _row("compact", mode=ref.MATRIX, **PLAIN8, adapt=1, comp_tab=1, comp_words=words - bayer_words, **BAYER8)
        rows[name + "_over_matrix"] = _row("compact", mode=ref.MATRIX, **PLAIN8, adapt=1, comp_tab=1, comp_words=words - bayer_words + 1, **BAYER8)
    rows["compact_needs_adapt"] = _row("fast", **PLAIN8, cell_perm=1, comp_tab=1, comp_words=9792)
    rows["compact_forced"] = _row("compact", **PLAIN8, cell_perm=1, comp_tab=1, comp_words=9792, force_compact=1)
    rows["compact_switched_off"] = _row("lean", **PLAIN8, adapt=1, comp_tab=1, comp_words=9792, no_compact_kernel=1)
    # float palettes: what the float kernels stage (table + records + lut_in), and the one-byte table of compact_float
    staged = (ref.LDS_BYTES - 256 * 16 - 256) // 4
    rows["float_staged_exact"] = _row("lean_float", is_integer=0, ftab=1, ftab_words=staged)
    rows["float_staged_over"] = _row("brute", is_integer=0, ftab=1, ftab_words=staged + 1)
    cf = (ref.LDS_BYTES - ref.K_CF_TAB_AT) // 4
    rows["compact_float_exact"] = _row("compact_float", is_integer=0, ftab=1, ftab_words=20000, comp_tab=1, comp_words=cf)
    rows["compact_float_over"] = _row("lean_float", is_integer=0, ftab=1, ftab_words=20000, comp_tab=1, comp_words=cf + 1)
    rows["float_matrix_no_fpad"] = _row("brute", mode=ref.MATRIX, is_integer=0, ftab=1, ftab_words=20000, m=1, th_h=8, th_w=8)
    # a single colour is nearest-only whatever was asked for
    rows["one_colour_matrix"] = _row("brute", K=1, mode=ref.MATRIX, **BAYER8)
    rows["one_colour_ign"] = _row("brute", K=1, mode=ref.IGN)
    rows["one_colour_float"] = _row("brute", K=1, mode=ref.MATRIX, is_integer=0, **BAYER8)
    # the traversal queue of the fix-up pass
    rows["n_inner_64"] = _row("lean", **PLAIN8, n_inner=64)
    rows["n_inner_65"] = _row("lean", **PLAIN8, n_inner=65)
    # geometry the tile kernels do not take; 24 frames of 3840 x 2160 on all 256 CUs
    rows["negative_y0"] = _row("cell", **PLAIN8, y0=-1)
    rows["negative_x0_partly_staged"] = _row("brute", cell_tab=1, tab_words=4096 * 8, tab_total=4096 * 8 + 8, x0=-3)
    rows["px_2_30"] = _row("lean", **PLAIN8, n_px=1 << 30, hw=1 << 30, w=1 << 15, n_cus=256)
    rows["px_over_2_30"] = _row("cell", **PLAIN8, n_px=(1 << 30) + 4, hw=(1 << 30) + 4, w=(1 << 15) + 1, n_cus=256)
    for mode in MODES:
        rows[f"4k_plain4_mode{mode}"] = _row("lean" if mode else "fast", mode=mode, **PLAIN8, cell_tab4=1, tab4_words=4096 * 4, cell_perm=1,
                                             cell_perm4=1, n_wide4=2, n_px=24 * 3840 * 2160, hw=3840 * 2160, w=3840, n_cus=256, **BAYER8)
    return rows


def _line(i, p):
    return "plan %d %s" % (i, " ".join(str(p[k]) for k in ref.PLAN_FIELDS))


def _key(p):
    return (p["family"], p["mode"], p["bw"], p["adapt"], p["warp"], p["half"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    tmp = tmp_path_factory.mktemp("orderedplan")

    def run(cases):
        """cases: [(facts, switches)] -> the lines the stand-alone build prints for them"""
        rec = np.array([[f[k] for k in ref.FACT_FIELDS] + [sw[k] for k in ref.SWITCH_FIELDS] for f, sw in cases], dtype=np.int64).astype("<i4")    # (every value is below 2^31)
        path = tmp / "cases.bin"
        rec.tofile(path)
        env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        r = subprocess.run([os.path.join(CSRC, "build", "host_asan"), "orderedplan", str(path), str(len(cases))], capture_output=True,
                           text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        return r.stdout.strip().split("\n")
    return run


def test_record_layout_matches_the_header():
    """The harness reads the two structs as they are declared: the field lists of the reference must be the header's."""
    import re
    with open(os.path.join(CSRC, "ordered_plan.h")) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    for struct, fields in (("OrderedFacts", ref.FACT_FIELDS), ("OrderedSwitches", ref.SWITCH_FIELDS)):
        body = re.search(r"struct %s \{(.*?)\};" % struct, text, re.S).group(1)
        names = [n for decl in re.findall(r"u?int32_t ([^;]*);", body) for n in re.split(r",\s*", decl.strip())]
        assert tuple(names) == fields, (struct, names)
        assert not re.sub(r"u?int32_t [^;]*;", "", body).strip(), struct     # 32-bit members only: no padding


def test_grid_reaches_every_kernel_and_the_planner_agrees(harness):
    cases = list(_grid())
    want = [ref.plan(f, sw) for f, sw in cases]
    reached = {_key(p) for p in want}
    assert {k[0] for k in reached} == FAMILIES, FAMILIES - {k[0] for k in reached}
    assert reached == KERNELS, (sorted(KERNELS - reached), sorted(reached - KERNELS))
    got = harness(cases)
    assert len(got) == len(cases)
    for i, (line, p) in enumerate(zip(got, want)):
        if line != _line(i, p):
            pytest.fail("case %d: planner says\n  %s\nreference says\n  %s\nfacts %r\nswitches %r" % ((i, line, _line(i, p)) + cases[i]))


def test_named_boundary_rows(harness):
    rows = _named()
    cases = [(f, sw) for _, f, sw in rows.values()]
    want = [ref.plan(f, sw) for f, sw in cases]
    for (name, (family, _, _)), p in zip(rows.items(), want):
        assert p["family"] == family, (name, p)
    by = dict(zip(rows, want))
    # what each boundary decides, beyond the family
    assert (by["lean_thr_exact"]["mode"], by["lean_thr_over"]["mode"]) == (1, 2)
    assert [by[n]["half"] for n in ("half_tab_exact", "half_tab_over", "half_tab_exact_matrix", "half_tab_over_matrix",
                                    "half_tab_exact_switched_off")] == [1, 0, 1, 0, 0]
    assert (by["half_tab_exact"]["grid"], by["half_tab_over"]["grid"]) == (16, 8)
    assert (by["fast_thr_exact"]["mode"], by["fast_thr_over"]["mode"]) == (1, 2)
    assert [by[n]["half"] for n in ("compact_half_exact", "compact_half_over", "compact_half_exact_matrix", "compact_half_over_matrix")] == [1, 0, 1, 0]
    assert [by[n]["mode"] for n in ("compact_full_exact_matrix", "compact_full_over_matrix")] == [1, 2]
    assert [by[n]["mode"] for n in ("one_colour_matrix", "one_colour_ign", "one_colour_float")] == [0, 0, 0]
    assert (by["n_inner_64"]["fix_big_queue"], by["n_inner_65"]["fix_big_queue"]) == (0, 1)
    p = by["4k_plain4_mode1"]       # two workgroups per CU: 512 x 4096 pixels ahead = 546 rows and 512 columns of 3840
    assert (p["bw"], p["half"], p["mode"], p["grid"], p["n_tiles"], p["adv_y"], p["adv_x"], p["fix_mode"], p["fix_grid"]) == \
        (4, 1, 1, 512, 48600, 546, 512, 2, 256)
    got = harness(cases)
    assert len(got) == len(cases)
    for i, (name, line, p) in enumerate(zip(rows, got, want)):
        assert line == _line(i, p), name
