"""CPU tier of the choice of the fine kernel's instance (dither_pie_amd/csrc/ordered_fine.h: choose_fine -- what launch_ordered asks after
plan_ordered: does ordered_fine_kernel take the call over, at which key level, on which table -- and fine_instance, the instances a build
has).

`finechoice` of the stand-alone host_asan build prints, for records of plan facts, the tables of a palette and the switches, the plan's
family, (fine, keys, sub) and whether the product and the experiments build have that instance.  Compared case by case with a
restatement that composes the restatements of the parts (fine_replaces: test_ordered_fine_cpu.py; fine_keys_level:
test_ordered_fine_keys_cpu.py; fine_sub_level: fine_sub_ref.py) by the rules of the choice, written from them and not from the C++:
    fine_plain = fine_replaces(plan, F) and not no_fine                     F = the plain table and the thresholds
    sub_only   = no plain table, a two-level one, fine_plan_ok(plan), not no_fine
    keys       = min(fine_keys_level(F), keys_cap) if fine_plain else (min(1, keys_cap) if sub_only else 0)
    sub        = fine_sub_level(two-level table present and (fine_plain or sub_only), its sizes, thresholds, keys, sub_cap)
    fine       = fine_plain or sub != 0;   keys is reported as 0 where fine is
over plans of every family x tables present and absent, at the budget's edges x three threshold matrices x every switch setting."""
import itertools

import numpy as np

import fine_sub_ref as fs
import ordered_plan_ref as ref
from test_ordered_fine_cpu import BASE, BAYER8, NO_SWITCH, PLAIN8, fine_replaces, harness  # noqa: F401  (harness: the fixture)
from test_ordered_fine_keys_cpu import fine_keys_level

TABLE_FIELDS = ("plain", "n_win", "n_wide", "sub", "sub_win", "sub_wide", "thr_bytes")
FSWITCH_FIELDS = ("no_fine", "keys_cap", "sub_cap")
PRODUCT = dict(no_fine=0, keys_cap=1, sub_cap=2)       # kFineKeysShipped, kFineSubShipped


def fine_plan_ok(p):
    return (p["family"] == "lean" and p["mode"] == 1 and p["bw"] == 8 and p["table"] == "plain8" and not p["adapt"] and not p["warp"] and
            not p["half"])


def choose_fine(p, t, sw):
    F = dict(present=t["plain"], n_win=t["n_win"], n_wide=t["n_wide"], thr_bytes=t["thr_bytes"])
    fine_plain = bool(fine_replaces(p, F)) and not sw["no_fine"]
    sub_only = bool(not t["plain"] and t["sub"] and fine_plan_ok(p) and not sw["no_fine"])
    keys = min(fine_keys_level(F), sw["keys_cap"]) if fine_plain else (min(1, sw["keys_cap"]) if sub_only else 0)
    sub = fs.fine_sub_level(dict(present=int(bool(t["sub"]) and (fine_plain or sub_only)), n_win=t["sub_win"], n_wide=t["sub_wide"],
                                 thr_bytes=t["thr_bytes"], keys=keys, cap=sw["sub_cap"]))
    fine = fine_plain or sub != 0
    return int(fine), keys if fine else 0, sub


def has_instance(keys, sub, experiments):
    """ordered_fine.h: fine_instance, restated as the lists the builds ship"""
    return (keys, sub) in ({(0, 0), (1, 0), (1, 2)} | ({(2, 0), (1, 1)} if experiments else set()))


def test_choice_against_the_restatement(harness, tmp_path):  # noqa: F811
    bayer8, m16, m64 = BAYER8, dict(BAYER8, th_h=16, th_w=16, tw_pad=19), dict(BAYER8, th_h=64, th_w=64, tw_pad=67)
    # (name, facts beside the thresholds, switches of the plan, integer thresholds, the plan wanted: family, mode)
    plans = (("lean8", PLAIN8, {}, True, ("lean", 1)),
             ("lean4", dict(PLAIN8, cell_tab4=1, tab4_words=4096 * 4), {}, True, ("lean", 1)),
             ("lean_f32", PLAIN8, {}, False, ("lean", 2)),
             ("fast", dict(PLAIN8, cell_perm=1, n_wide=3), dict(fast_all=1), True, ("fast", None)),
             ("compact", dict(PLAIN8, comp_tab=1, comp_words=9000), dict(force_compact=1), True, ("compact", None)),
             ("cell", dict(PLAIN8, aligned=0), {}, True, ("cell", None)),
             ("brute", {}, {}, True, ("brute", None)))
    # the most windows that fit beside Bayer 8x8 and 370 rows, as in test_ordered_fine_sub_cpu.py: test_level_function
    edge = (fs.LEAN_TAB_BYTES - 8 * 11 * 4 - fs.FINE_CELLS * 2 - 370 * 16) // 40
    sub_sizes = ((2063, 370), (edge, 370), (edge + 1, 370), (1500, 513))
    switches = [dict(no_fine=a, keys_cap=b, sub_cap=c) for a, b, c in itertools.product((0, 1), (0, 1, 2), (0, 1, 2))]
    cases = []
    for (name, tab, psw, int_thr, wanted), thr, plain, sub, (sub_win, sub_wide), fsw in itertools.product(
            plans, (bayer8, m16, m64), (1, 0), (1, 0), sub_sizes, switches):
        f = dict(BASE, **tab, **(thr if int_thr else dict(thr, m=0, mpad=0)))
        t = dict(plain=plain, n_win=1793, n_wide=370, sub=sub, sub_win=sub_win, sub_wide=sub_wide, thr_bytes=f["th_h"] * f["tw_pad"] * 4)
        cases.append((name, wanted, f, dict(NO_SWITCH, **psw), t, fsw))
    plan_of = {}
    for name, wanted, f, sw, t, fsw in cases:
        key = (name, f["th_h"])
        if key not in plan_of:
            plan_of[key] = ref.plan(f, sw)
            assert plan_of[key]["family"] == wanted[0] and wanted[1] in (None, plan_of[key]["mode"]), (name, plan_of[key])
    want = [choose_fine(plan_of[(name, f["th_h"])], t, fsw) for name, wanted, f, sw, t, fsw in cases]

    # the case set reaches what it is meant to reach
    assert {(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 1, 1), (1, 1, 2)} == set(want)

    def pick(name, thr_h, **kw):
        """the answers of the cases of one plan whose tables and switches have these values"""
        got = [w for w, (n, _, f, _, t, fsw) in zip(want, cases) if n == name and f["th_h"] == thr_h and all(dict(t, **fsw)[k] == v for k, v in kw.items())]
        assert got
        return got
    sub_only = dict(plain=0, sub=1, sub_win=2063, sub_wide=370)
    assert pick("lean8", 8, **sub_only, **PRODUCT) == [(1, 1, 2)]
    assert pick("lean8", 8, **sub_only, **dict(PRODUCT, keys_cap=0)) == [(0, 0, 0)]
    assert pick("lean8", 8, plain=1, sub=1, sub_win=edge, sub_wide=370, **PRODUCT) == [(1, 1, 2)]
    # one window over the budget: what the plain table alone gives; nothing without it
    assert pick("lean8", 8, plain=1, sub=1, sub_win=edge + 1, sub_wide=370, **PRODUCT) == pick("lean8", 8, plain=1, sub=0, sub_win=edge + 1, sub_wide=370, **PRODUCT) == [(1, 1, 0)]
    assert pick("lean8", 8, plain=0, sub=1, sub_win=edge + 1, sub_wide=370, **PRODUCT) == [(0, 0, 0)]
    assert pick("lean8", 8, plain=1, sub=1, sub_win=1500, sub_wide=513, **PRODUCT) == [(1, 1, 0)]
    for name in ("lean4", "lean_f32", "fast", "compact", "cell", "brute"):
        assert set(pick(name, 8)) == {(0, 0, 0)}, name
    for w, (_, _, _, _, _, fsw) in zip(want, cases):
        assert has_instance(w[1], w[2], True), (w, fsw)
        assert fsw != PRODUCT or has_instance(w[1], w[2], False), (w, fsw)

    rec = np.array([[f[k] for k in ref.FACT_FIELDS] + [sw[k] for k in ref.SWITCH_FIELDS] + [t[k] for k in TABLE_FIELDS] + [fsw[k] for k in FSWITCH_FIELDS]
                    for _, _, f, sw, t, fsw in cases], dtype=np.int64).astype("<i4")
    rec.tofile(tmp_path / "cases.bin")
    got = harness("finechoice", tmp_path / "cases.bin", len(cases))
    assert len(got) == len(cases)
    for i, (line, w, (name, _, f, _, t, fsw)) in enumerate(zip(got, want, cases)):
        family = plan_of[(name, f["th_h"])]["family"]
        assert line == "choice %d %s %d %d %d %d %d" % (i, family, *w, has_instance(w[1], w[2], False), has_instance(w[1], w[2], True)), (i, line, w, t, fsw)
