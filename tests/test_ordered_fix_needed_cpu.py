"""CPU tier of the decision whether a call of the ordered dither keeps its fix-up pass (dither_pie_amd/csrc/ordered_fix.h: fix_needed --
what launch_ordered asks after plan_ordered and choose_fine: may the reset of the flagged-tile count and the fix-up launch be left out).

`fixneeded` of the stand-alone host_asan build prints 0 / 1 for records of one FixFacts and one FixSwitches.  Compared case by case with
tests/ordered_fix_ref.py over the product of every family x fine or not x integer / float x accelerator present or not x every table kind x
slow-block counts {0, 1} x n_exc {-1, 0, 5} x the switch; and the two outcomes that matter are asserted by name: the facts of
palr(256, 7) -- the headline's palette: a lean plan the fine kernel replaces, plain 8-entry table without marker blocks, a short exception
list -- give no fix-up pass, the same palette with one slow block keeps it."""
import itertools

import numpy as np

import ordered_fix_ref as fx
from test_ordered_fine_cpu import harness  # noqa: F401  (the fixture)

OFF, ON = dict(always_fixup=0), dict(always_fixup=1)
# what launch_ordered sees for palr(256, 7) with Bayer 8x8 (n_exc: a few dozen four-way ties at most; its value beyond the sign is not read)
PALR256 = dict(family="lean", fine=1, is_integer=1, accel=1, table="plain8", slow_blocks=0, n_exc=5)


def test_the_two_outcomes_by_name():
    assert fx.fix_needed(PALR256, OFF) is False
    assert fx.fix_needed(dict(PALR256, slow_blocks=1), OFF) is True
    # ... and what else keeps the pass for that palette: the switch, an overflowed list; the lean kernel itself may drop it as well
    assert fx.fix_needed(PALR256, ON) is True
    assert fx.fix_needed(dict(PALR256, n_exc=-1), OFF) is True
    assert fx.fix_needed(dict(PALR256, n_exc=0), OFF) is False
    assert fx.fix_needed(dict(PALR256, fine=0), OFF) is False
    for table in ("plain4", "warped"):
        assert fx.fix_needed(dict(PALR256, fine=0, table=table), OFF) is False
        assert fx.fix_needed(dict(PALR256, fine=0, table=table, slow_blocks=1), OFF) is True


def test_fix_needed_against_the_restatement(harness, tmp_path):  # noqa: F811
    cases = [(dict(family=fam, fine=fine, is_integer=integer, accel=accel, table=table, slow_blocks=slow, n_exc=n_exc), dict(always_fixup=sw))
             for fam, fine, integer, accel, table, slow, n_exc, sw in itertools.product(fx.FAMILIES, (0, 1), (1, 0), (1, 0), fx.TABLES, (0, 1),
                                                                                        (-1, 0, 5), (0, 1))]
    want = [fx.fix_needed(f, sw) for f, sw in cases]
    # the case set reaches both outcomes, and the pass is dropped for nothing but a lean plan of an integer palette with its accelerator
    assert set(want) == {False, True}
    for (f, sw), w in zip(cases, want):
        if not w:
            assert f["family"] == "lean" and f["is_integer"] and f["accel"] and f["slow_blocks"] == 0 and f["n_exc"] >= 0 and not sw["always_fixup"]
    assert (PALR256, OFF) in cases and (dict(PALR256, slow_blocks=1), OFF) in cases

    np.array([fx.record(f, sw) for f, sw in cases], dtype=np.int64).astype("<i4").tofile(tmp_path / "cases.bin")
    got = harness("fixneeded", tmp_path / "cases.bin", len(cases))
    assert len(got) == len(cases)
    for i, (line, w, (f, sw)) in enumerate(zip(got, want, cases)):
        assert line == "fix %d %s %d" % (i, f["family"], int(w)), (i, line, f, sw)
    assert got[cases.index((PALR256, OFF))].endswith(" lean 0")
    assert got[cases.index((dict(PALR256, slow_blocks=1), OFF))].endswith(" lean 1")
