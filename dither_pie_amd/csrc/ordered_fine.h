// Whether ordered_fine_kernel (ordered.hip) serves a call in place of the kernel plan_ordered chose, and the LDS budget of its
// table: plain C++17 like ordered_plan.h, included by ordered.hip and accel.hip and compiled on its own into the sanitizer
// harness (host_sanitize.cpp, `fineplan`), where tests/test_ordered_fine_cpu.py compares it case by case with a Python
// restatement.  plan_ordered, OrderedFacts and their record format are what they were: the fine kernel is a refinement of one
// row of the plan -- the lean kernel on the plain 8-entry table with integer thresholds in LDS -- and takes that row's grid,
// tile stride and fix-up pass unchanged.
#pragma once
#include <cstdint>

#include "ordered_plan.h"

namespace dp {

// What the kernel stages (host_logic.h: FineTable::lds_image), thresholds behind it, the lean kernel's queues at the top:
//   quads A [n_win x 16 B] | flat lists of the wide cells [n_wide x 64 B] | pairs B [n_win x 8 B] | window of every cell
//   [32768 x 2 B] | cell numbers of the wide cells [kFineIds x 2 B] | integer thresholds
constexpr int64_t fine_table_bytes(const int n_win, const int n_wide)
{
    return (int64_t)n_win * (kFineWindow * 4) + (int64_t)n_wide * kWideList * 4 + kFineCells * 2 + kFineIds * 2;
}
// what the builder (accel.hip) asks the packer to stay within: room is left for the thresholds of a 16 x 16 matrix (rows padded
// by three); a larger matrix that no longer fits keeps the lean kernel (fine_replaces).  Wide cells: kFineIds at most -- 1.6 %
// of the cells; their pixels leave the main path.
constexpr bool fine_table_fits(const int n_win, const int n_wide)
{
    return fine_table_bytes(n_win, n_wide) + 16 * 19 * 4 <= kLeanTabBytes;
}

struct FineFacts {  // 32-bit members: also the record format of the test harness
    int32_t present;    // the palette has a fine table
    int32_t n_win, n_wide;
    int32_t thr_bytes;  // the padded integer thresholds: th_h * tw_pad * 4
};

inline bool fine_replaces(const OrderedPlan &p, const FineFacts &f)
{
    return f.present != 0 && p.family == kFamLean && p.mode == 1 && p.bw == 8 && p.table == kTabPlain8 && !p.adapt && !p.warp && !p.half &&
           fine_table_bytes(f.n_win, f.n_wide) + (int64_t)f.thr_bytes <= kLeanTabBytes;
}

}  // namespace dp
