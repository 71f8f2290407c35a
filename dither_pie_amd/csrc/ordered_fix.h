// Whether a call of the ordered dither needs its fix-up pass at all: plain C++17 like ordered_plan.h and ordered_fine.h, included by
// ordered.hip and compiled on its own into the sanitizer harness (host_sanitize.cpp, `fixneeded`), where
// tests/test_ordered_fix_needed_cpu.py compares it case by case with tests/ordered_fix_ref.py.  OrderedPlan, OrderedFacts, FineChoice,
// FineTables and their record formats are what they were: this decision stands beside them.
//
// A call queues three dispatches: a 4-byte memset of the count of flagged wave tiles (Geo::dirty), the pass-1 kernel, and
// fixup_kernel, which reads the count and returns at once when it is 0.  Where no pixel can ever be flagged, the memset and the fix-up
// launch do nothing and launch_ordered leaves them out; ordered_fine_kernel's NOFLAGS instances also leave out the stores that clear
// the flag bitmap nobody reads then.
//
// Audit of the flag sources of the lean kernels and of the fine kernel that replaces one of them (ordered.hip):
//   ordered_lean_kernel   clear_flags per tile (clears only); flag_slow_pixel behind resolve_pixel's `slow` in the ADAPT in-place path
//                         and, through the queue, in lean_pixel_full
//   ordered_fine_kernel   clear_flags per tile (clears only); flag_slow_pixel behind resolve_pixel's `slow` in fine_pixel_full, on the
//                         plain 8-entry table in global memory (leaf_find_global<8>).  resolve_wide and resolve_window never flag:
//                         they pass a pixel on to resolve_pixel.
//   neither calls store_flags (the brute, cell, fast, compact and float kernels do).
// resolve_pixel sets `slow` in two places only:
//   1. `stuck` -- the descent ended on a 0xC0000000 marker block, a single colour with more candidates than a block holds -- on a
//      table of 8-entry blocks.  (leaf_step also says stuck below bit 0, but assemble_table (host_logic.h) writes the marker for every
//      box of size 1, so no split marker sits that deep.)  The markers of a table are counted while it is assembled: TableStats::n_slow,
//      kept as PalDev::n_slow_blocks for the plain 8-entry table wherever that table exists, and as PalDev::warp_slow_blocks for the
//      table over warped cells, which has markers of its own.  On 4-entry blocks `stuck` is resolved by a scan of the palette, never
//      flagged: launch_ordered passes 0 for the plain 4-entry table, whose markers PalDev does not count.
//   2. a tie code that names no outcome (3 for k = 1, 15 for k = 2) whose colour find_exception does not find.  accel_scan_kernel
//      (accel.hip) appends an entry to the exception list for every colour it gives such a code, so the colour is missing only if the
//      list overflowed: PalDev::n_exc < 0.  (A tie the kernel sees among its candidates where the scan saw none reads code 0.)
// Both are properties of the palette, fixed when the accelerator is built; frames, thresholds and geometry have no part in them.
#pragma once
#include <cstdint>

#include "ordered_plan.h"

namespace dp {

struct FixFacts {  // 32-bit members: also the record format of the test harness
    int32_t family;       // OrderedFamily of the plan
    int32_t fine;         // ordered_fine_kernel runs in place of the plan's kernel (FineChoice::fine)
    int32_t is_integer;   // PalDev::is_integer
    int32_t accel;        // the palette has its search accelerator (tables, tie codes, exception list)
    int32_t table;        // OrderedTable of the plan
    int32_t slow_blocks;  // 0xC0000000 marker blocks of THAT table that a kernel would flag a pixel for
    int32_t n_exc;        // PalDev::n_exc
};
struct FixSwitches {  // the product library: {0}
    int32_t always_fixup;  // experiments: DP_ALWAYS_FIXUP, the three dispatches whatever the palette
};

inline bool fix_needed(const FixFacts &f, const FixSwitches &sw)
{
    if (sw.always_fixup != 0) return true;
    if (f.family != kFamLean) return true;  // (the fine kernel replaces a lean plan: its family is this one)
    if (f.fine != 0 && f.table != kTabPlain8) return true;  // (not planned: its deferred path reads the plain 8-entry table)
    if (f.is_integer == 0 || f.accel == 0) return true;
    return f.slow_blocks != 0 || f.n_exc < 0;
}

}  // namespace dp
