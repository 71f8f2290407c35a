"""Which ordered-dither kernel serves a call: a Python statement of the decision `launch_ordered` took before it was split
into facts / plan / launch (dither_pie_amd/csrc/ordered.hip at the commit that added pattern dithering), transcribed from
that function branch by branch -- NOT from ordered_plan.h, which tests/test_ordered_plan_cpu.py checks against it.

`plan(facts, switches)` takes two dicts (FACT_FIELDS / SWITCH_FIELDS: what the launcher knows about the palette, the
thresholds and one chunk of frames; the five experiment switches) and returns the dict of PLAN_FIELDS.
"""

NEAREST, MATRIX, IGN = 0, 1, 2          # DP_MODE_* (include/ditherpie_hip.h)

FACT_FIELDS = ("mode", "K", "is_integer", "n_inner",
               "n_px", "hw", "w", "y0", "x0", "aligned",
               "cell_tab", "tab_words", "tab_total", "cell_tab4", "tab4_words",
               "warp_tab", "warp_words", "warp_total", "warp_bw", "warp_adapt",
               "adapt", "cell_perm", "cell_perm4", "n_wide", "n_wide4",
               "comp_tab", "comp_words", "comp_warp", "ftab", "ftab_words",
               "m", "mpad", "fpad", "th_h", "th_w", "tw_pad", "n_cus")
SWITCH_FIELDS = ("lean_no_half", "fast_all", "force_compact", "no_compact_kernel", "compact_no_half")
PLAN_FIELDS = ("family", "mode", "bw", "adapt", "warp", "half", "table", "grid", "block", "n_tiles", "n_words", "adv_y", "adv_x",
               "lds_bytes", "fix_mode", "fix_big_queue", "fix_grid")

# the LDS budgets of the kernels, as the parent's ordered.hip spelled them
K_BLOCK = 256
K_CELL_BLOCK = 1024
K_LEAN_LDS_WORDS = 160 * 1024 // 4
K_LEAN_QUEUE = 128
K_LEAN_QUEUE_WORDS = (K_CELL_BLOCK // 64) * K_LEAN_QUEUE
K_LEAN_TAB_BYTES = (K_LEAN_LDS_WORDS - K_LEAN_QUEUE_WORDS) * 4
K_LEAN_HALF_LDS_WORDS = 80 * 1024 // 4
K_LEAN_HALF_QUEUE = 112
K_LEAN_HALF_TAB_BYTES = (K_LEAN_HALF_LDS_WORDS - (K_CELL_BLOCK // 64) * K_LEAN_HALF_QUEUE) * 4
K_WARP_LUT_BYTES = 768
K_COMPACT_HALF_WORDS = 80 * 1024 // 4
K_COMPACT_TAB_AT = 256 * 8 + K_WARP_LUT_BYTES
K_CF_TAB_AT = 256 * 16 + 256
K_WIDE_LIST = 16
K_FAST_QUEUE = 128
K_QUEUE_SMALL = 64
LDS_BYTES = 4 * K_LEAN_LDS_WORDS


def fast_fixed_bytes(bw, n_wide):
    """What ordered_fast_kernel stages whatever the mode: 4096 cell blocks, the flat lists of the split cells, two queues."""
    return 4096 * bw * 4 + n_wide * K_WIDE_LIST * 4 + 2 * (K_CELL_BLOCK // 64) * K_FAST_QUEUE * 4


def plan(f, sw):
    mode = f["mode"]
    if f["K"] == 1:
        mode = NEAREST
    hw, w, cus = f["hw"], f["w"], f["n_cus"]
    integer = f["is_integer"] != 0
    aligned = f["aligned"] != 0
    groups = (f["n_px"] + 3) // 4
    blocks = (groups + K_BLOCK - 1) // K_BLOCK
    thr_bytes = f["th_h"] * f["tw_pad"] * 4
    out = dict(family="brute", bw=8, adapt=0, warp=0, half=0, table="plain8", grid=blocks, block=K_BLOCK, n_tiles=0,
               n_words=blocks * (K_BLOCK // 64) * 4, adv_y=0, adv_x=0, lds_bytes=0)

    def tiles(grid):
        out["n_tiles"] = (groups + K_CELL_BLOCK - 1) // K_CELL_BLOCK
        out["n_words"] = out["n_tiles"] * (K_CELL_BLOCK // 64) * 4
        out["block"] = K_CELL_BLOCK
        out["grid"] = min(out["n_tiles"], cus * grid)
        adv = (out["grid"] * K_CELL_BLOCK * 4) % hw
        out["adv_y"], out["adv_x"] = adv // w, adv % w

    int_thr_ok = f["m"] != 0 and f["th_h"] * f["th_w"] <= 256
    warp = f["warp_tab"] != 0
    small = f["warp_bw"] == 4 if warp else f["cell_tab4"] != 0
    lean_tab_bytes = 4 * f["warp_words"] + K_WARP_LUT_BYTES if warp else 4 * (f["tab4_words"] if small else f["tab_words"])
    geo_ok = (integer and (warp or small or f["cell_tab"] != 0) and aligned and f["y0"] >= 0 and f["x0"] >= 0 and
              f["n_px"] <= (1 << 30))
    lean_geo = geo_ok and lean_tab_bytes <= K_LEAN_TAB_BYTES
    int_lean = f["mpad"] != 0 and lean_tab_bytes + thr_bytes <= K_LEAN_TAB_BYTES
    lean_ok = lean_geo and (mode == NEAREST or mode == IGN or (mode == MATRIX and (int_lean or f["fpad"] != 0)))
    whole_tab = f["cell_tab"] != 0 and f["tab_total"] == f["tab_words"]
    if integer and (lean_ok or whole_tab):
        half = (lean_ok and small and not warp and not sw["lean_no_half"] and
                lean_tab_bytes + (thr_bytes if mode == MATRIX and int_lean else 0) <= K_LEAN_HALF_TAB_BYTES)
        tiles(2 if half else 1)
        table = "warped" if warp else ("plain4" if small else "plain8")
        adapt = f["warp_adapt"] != 0 if warp else (not small and f["adapt"] != 0)
        perm = f["cell_perm4"] if small else f["cell_perm"]
        fast_fixed = fast_fixed_bytes(4 if small else 8, f["n_wide4"] if small else f["n_wide"])
        int_fast = f["mpad"] != 0 and fast_fixed + thr_bytes <= LDS_BYTES
        fast_mode = mode == NEAREST or sw["fast_all"]
        fast_ok = (fast_mode and geo_ok and not warp and not adapt and perm != 0 and fast_fixed <= LDS_BYTES and
                   (mode == NEAREST or mode == IGN or (mode == MATRIX and (int_fast or f["fpad"] != 0))))
        comp_base = K_COMPACT_TAB_AT + 4 * f["comp_words"] if f["comp_tab"] else 0
        int_comp = mode == MATRIX and f["mpad"] != 0 and comp_base + thr_bytes <= LDS_BYTES
        comp_bytes = comp_base + (thr_bytes if int_comp else 0)
        comp_ok = (f["comp_tab"] != 0 and geo_ok and (adapt or sw["force_compact"]) and comp_bytes <= LDS_BYTES and
                   (mode == NEAREST or mode == IGN or (mode == MATRIX and (int_comp or f["fpad"] != 0))) and
                   not sw["no_compact_kernel"])
        comp_half = comp_ok and comp_bytes <= 4 * K_COMPACT_HALF_WORDS and not sw["compact_no_half"]

        def lean_kernel():
            if warp and small:
                return dict(bw=4, adapt=0, warp=1, half=0)
            if warp and adapt:
                return dict(bw=8, adapt=1, warp=1, half=0)
            if warp:
                return dict(bw=8, adapt=0, warp=1, half=0)
            if small and half:
                return dict(bw=4, adapt=0, warp=0, half=1)
            if small:
                return dict(bw=4, adapt=0, warp=0, half=0)
            if adapt:
                return dict(bw=8, adapt=1, warp=0, half=0)
            return dict(bw=8, adapt=0, warp=0, half=0)

        if comp_ok and mode in (NEAREST, IGN, MATRIX):
            tiles(2 if comp_half else 1)          # the compact kernel's own grid, and the tile stride again for it
            out.update(family="compact", warp=int(f["comp_warp"] != 0), half=int(comp_half))
            out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else (1 if int_comp else 2))
        elif fast_ok and (mode in (NEAREST, IGN) or (mode == MATRIX and (int_fast or f["fpad"] != 0))):
            out.update(family="fast", bw=4 if small else 8, table=table)
            out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else (1 if int_fast else 2))
        elif lean_geo and (mode in (NEAREST, IGN) or (mode == MATRIX and (int_lean or f["fpad"] != 0))):
            out.update(family="lean", table=table, **lean_kernel())
            out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else (1 if int_lean else 2))
        else:
            out.update(family="cell", lds_bytes=4 * (f["tab_words"] + 256))
            out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else (1 if int_thr_ok else 2))
    elif (not integer and f["ftab"] != 0 and aligned and f["y0"] >= 0 and f["x0"] >= 0 and
          f["ftab_words"] * 4 + f["K"] * 16 + 256 <= LDS_BYTES and (mode != MATRIX or f["fpad"] != 0)):
        cf_bytes = K_CF_TAB_AT + 4 * f["comp_words"] if f["comp_tab"] else 0
        cf_ok = f["comp_tab"] != 0 and cf_bytes <= LDS_BYTES and not sw["no_compact_kernel"]
        tiles(1)
        out["family"] = "compact_float" if cf_ok else "lean_float"
        out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else 2)
    else:
        out["mode"] = 0 if mode == NEAREST else (3 if mode == IGN else (1 if integer and int_thr_ok else 2))
    out["fix_mode"] = {0: 0, 3: 3, 1: 2, 2: 2}[out["mode"]]
    out["fix_big_queue"] = int(f["n_inner"] > K_QUEUE_SMALL)
    out["fix_grid"] = min((out["n_words"] + K_BLOCK * 8 - 1) // (K_BLOCK * 8), cus)
    return out
