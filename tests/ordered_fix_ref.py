"""Whether a call of the ordered dither keeps its fix-up pass (dither_pie_amd/csrc/ordered_fix.h: fix_needed), restated from the
rule and not from the C++:

    the pass (and the reset of its count before the kernel) is left out exactly when
      * the plan's family is `lean` -- the fine kernel replaces a lean plan and changes nothing about that -- and a fine call runs on
        the plain 8-entry table,
      * the palette is an integer one with its accelerator,
      * the table the plan chose has no 0xC0000000 marker block that a kernel flags a pixel for (the launcher passes 0 for the plain
        4-entry table, whose markers are resolved by a scan), and
      * the exception list did not overflow (n_exc >= 0),
    and the DP_ALWAYS_FIXUP switch of the experiments build is off.

Used by tests/test_ordered_fix_needed_cpu.py (against the harness) and tests/test_gpu_ordered_one_launch.py (against the trace)."""

FAMILIES = ("brute", "cell", "fast", "lean", "compact", "lean_float", "compact_float")   # ordered_plan.h: OrderedFamily
TABLES = ("plain8", "plain4", "warped")                                                  # ordered_plan.h: OrderedTable
FACT_FIELDS = ("family", "fine", "is_integer", "accel", "table", "slow_blocks", "n_exc")
SWITCH_FIELDS = ("always_fixup",)


def fix_needed(f, sw):
    """f: dict of FACT_FIELDS with family and table as names; sw: dict of SWITCH_FIELDS"""
    can_skip = (f["family"] == "lean" and (not f["fine"] or f["table"] == "plain8") and bool(f["is_integer"]) and bool(f["accel"]) and
                f["slow_blocks"] == 0 and f["n_exc"] >= 0)
    return bool(sw["always_fixup"]) or not can_skip


def record(f, sw):
    """the int32 fields of one harness record"""
    return ([FAMILIES.index(f["family"]), int(f["fine"]), int(f["is_integer"]), int(f["accel"]), TABLES.index(f["table"]), f["slow_blocks"],
             f["n_exc"]] + [int(sw[k]) for k in SWITCH_FIELDS])
