// Whether ordered_fine_kernel (ordered.hip) serves a call in place of the kernel plan_ordered chose, and the LDS budget of its
// table: plain C++17 like ordered_plan.h, included by ordered.hip and accel.hip and compiled on its own into the sanitizer
// harness (host_sanitize.cpp, `fineplan`), where tests/test_ordered_fine_cpu.py compares it case by case with a Python
// restatement.  plan_ordered, OrderedFacts and their record format are what they were: the fine kernel is a refinement of one
// row of the plan -- the lean kernel on the plain 8-entry table with integer thresholds in LDS -- and takes that row's grid,
// tile stride and fix-up pass unchanged.  choose_fine at the end is what launch_ordered calls: which instance of the kernel, if any.
#pragma once
#include <algorithm>
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

// Key levels of the kernel (ordered.hip: ordered_fine_kernel<MODE, KEYS>).  A candidate key is (|c|^2 << 8) + 4 * position
// - 2 * (x . c) << 8; everything but the last term is a constant of the window position.  Level 0 computes it per pixel from the
// staged image above (four instructions per key).  Levels 1 and 2 build another layout in LDS from the same global image, with that
// constant N next to the colour (two instructions per key), and leave the flat lists of the wide cells in global memory:
//   quads A {c0..c3} [n_win x 16 B] | their norms {N0..N3} [n_win x 16 B] | level 1: pairs B [n_win x 8 B], level 2: records B'
//   {c4, c5, N4, N5} [n_win x 16 B] | window of every cell | cell numbers of the wide cells | integer thresholds
constexpr int64_t fine_keys_bytes(const int level, const int n_win)
{
    return (int64_t)n_win * (level == 2 ? 48 : 40) + kFineCells * 2 + kFineIds * 2;
}
// the highest level whose layout fits next to the thresholds; consulted where fine_replaces says yes (tests/test_ordered_fine_keys_cpu.py)
inline int fine_keys_level(const FineFacts &f)
{
    if (f.present == 0) return 0;
    for (int level = 2; level >= 1; --level)
        if (fine_keys_bytes(level, f.n_win) + (int64_t)f.thr_bytes <= kLeanTabBytes) return level;
    return 0;
}

// The highest level the library launches by itself.  Level 2 fits the headline's table, but measured slower than level 1 on MI355X:
// once the keys are two instructions the LDS pipe limits the kernel as much as the vector issue does, and the 16-byte reads of B'
// cost it more than the four instructions they save (profiles/experiments/fine_keys_levels.md).  The level-2 instance
// exists in the experiments build only (DP_FINE_KEYS_MAX=2).
constexpr int kFineKeysShipped = 1;

// The two-level table (host_logic.h: fine_pack_sub; ordered.hip: ordered_fine_kernel<MODE, 1, SUB>).  A wide cell's entry of `off` is
// a tag plus its rank among the wide cells, and a row of eight window numbers serves its 4-wide sub-cells, so that only the pixels
// of the few sub-cells that are still wide leave the main path.  Key level 1 only.  LDS:
//   quads A [n_win x 16 B] | their norms [n_win x 16 B] | pairs B [n_win x 8 B] | window or tag of every cell [32768 x 2 B] | rows
//   [n_wide x 16 B] | integer thresholds
// (the sorted cell numbers of the wide cells are not staged: the tag is the rank), and the image in global memory, which also holds
// the flat lists, is  A | flat lists [n_wide x 64 B] | B | off | rows.  SUB 2 stages the same parts in another order, `off` | rows |
// quads A | norms | pairs B | thresholds, and the tags ready for use (kFineRowsAt, fine_stage_tag below); the bytes in all are the same.
constexpr int64_t fine_sub_bytes(const int n_win, const int n_wide)
{
    return (int64_t)n_win * 40 + kFineCells * 2 + (int64_t)n_wide * 16;
}
constexpr int64_t fine_sub_image_bytes(const int n_win, const int n_wide)
{
    return (int64_t)n_win * (kFineWindow * 4) + (int64_t)n_wide * (kWideList * 4 + 16) + kFineCells * 2;
}
// the room beside the two-level table: the most threshold bytes a call may bring and still run on it (fine_sub_level; host.cpp
// packs the other table for a call that brings more)
constexpr int64_t fine_sub_room(const int n_win, const int n_wide)
{
    return kLeanTabBytes - fine_sub_bytes(n_win, n_wide);
}
// what the builder asks fine_pack_sub to stay within: the thresholds of a 16 x 16 matrix beside the table as in fine_table_fits, and
// the image within the table's place in the accelerator's blob.  All or nothing: a palette whose joint pack does not fit gets no
// two-level table and keeps what fine_pack gives it.
constexpr bool fine_sub_fits(const int n_win, const int n_wide)
{
    return n_wide <= kFineIds && fine_sub_bytes(n_win, n_wide) + 16 * 19 * 4 <= kLeanTabBytes && fine_sub_image_bytes(n_win, n_wide) <= kLeanTabBytes;
}

struct FineSubFacts {  // 32-bit members: the record format of the test harness (`finesublevel`); FineFacts stays what it is
    int32_t present;    // the palette has a two-level table
    int32_t n_win, n_wide;
    int32_t thr_bytes;
    int32_t keys;       // the key level the call runs at (after any cap): the SUB instances exist at level 1 only
    int32_t cap;        // the highest SUB level allowed (kFineSubShipped, or DP_FINE_SUB_MAX in the experiments build)
};
// The SUB level of a call that fine_replaces has accepted (or would, given today's table): 0 is today's kernel on today's table.
//   1: the main loop is today's (a tag is staged as window 0); the deferred path ranks a wide cell's pixel on its sub-cell's window
//      in LDS.  The cheaper partner of the A/B: an instance of the experiments build only.
//   2: the main loop replaces a tagged window number by the row's entry for the pixel's sub-cell.
inline int fine_sub_level(const FineSubFacts &f)
{
    if (f.present == 0 || f.keys != 1 || f.cap < 1 || f.n_wide > kFineIds) return 0;
    return (int64_t)f.thr_bytes <= fine_sub_room(f.n_win, f.n_wide) ? (f.cap < 2 ? 1 : 2) : 0;
}
// whether the plan is one the fine kernels take over at all (the first half of fine_replaces)
inline bool fine_plan_ok(const OrderedPlan &p)
{
    return p.family == kFamLean && p.mode == 1 && p.bw == 8 && p.table == kTabPlain8 && !p.adapt && !p.warp && !p.half;
}

// The highest SUB level the library launches by itself.  Level 2 measured 6-7 % above today's kernel on the headline, every run
// above every run of the parent; level 1 measured exactly today's time -- it makes a wide pixel's drain cheaper, not rarer -- and
// exists in the experiments build only (DP_FINE_SUB_MAX=1; DESIGN 4.1, profiles/experiments/fine_sub_levels.md).
constexpr int kFineSubShipped = 2;

// ---- the address arithmetic of the main loop, shared with the deferred path and, as plain C++, with the test harness
// (host_sanitize.cpp `fineaddr`; tests/test_ordered_fine_addr_cpu.py) -----------------------------------------------------
// a . b over the four bytes, plus c: one v_dot4_u32_u8 on the device
DP_HD inline uint32_t fine_udot4(const uint32_t a, const uint32_t b, const uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    uint32_t s = c;
    for (int i = 0; i < 4; ++i) s += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return s;
#endif
}
// byte offset of the window number of x's cell, from `base`: 2 * fine_cell = 2 r5 + 64 g5 (the dot product) + (b5 << 11) (its
// accumulator); bits 24-31 of x are ignored.  Five instructions, four where base is 0.  (The byte weights are a parameter so that
// the kernel can say which register file holds them; so in fine_row_offset.)
constexpr uint32_t kFineCellWeights = 0x00004002u, kFineSubWeights = 0x00080402u;
DP_HD inline uint32_t fine_cell_offset(const uint32_t x, const uint32_t base = 0u, const uint32_t weights = kFineCellWeights)
{
    const uint32_t z = (x >> 3) & 0x1f1f1fu;
#if defined(__HIP_DEVICE_COMPILE__)
    // byte 2 of z shifted in one instruction (the compiler makes a shift and a mask of x from the line below)
    uint32_t hi;
    asm("v_lshlrev_b32_sdwa %0, 11, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(hi) : "v"(z));
#else
    const uint32_t hi = (z >> 16) << 11;
#endif
    return fine_udot4(z, weights, hi + base);
}
// SUB 2 stages `off` first and the rows right behind it (the global image and the other levels are what they were): the base of
// `off` is no operand at all, and the rows sit at a constant address.
constexpr uint32_t kFineRowsAt = (uint32_t)kFineCells * 2u;
// ... and stages the tag of a wide cell ready for use: bit 15 | rank << 4, the row's offset
DP_HD inline uint32_t fine_stage_tag(const uint32_t tag) { return (uint32_t)kFineSubTag | ((tag & (uint32_t)(kFineIds - 1)) << 4); }
DP_HD inline uint32_t fine_tag_rank(const uint32_t staged) { return (staged >> 4) & (uint32_t)(kFineIds - 1); }
// two window numbers at a time, as the stager meets them (a tagged half has bit 15 set)
DP_HD inline uint32_t fine_stage_tags2(const uint32_t v)
{
    const uint32_t t = v & 0x80008000u, m = (t >> 15) * 0xffffu;
    return (v & ~m) | (m & (t | ((v & 0x01ff01ffu) << 4)));
}
static_assert(kFineIds == 512, "fine_stage_tags2: nine bits of rank");
// the row entry of a staged tag for the colour x, less the tag bit: tag + 2 * sub-cell, the sub-cell from bit 2 of r, g and b
// (host_logic.h: fine_sub_cell) as a dot product with the byte weights 2, 4, 8 and the tag as its accumulator
DP_HD inline uint32_t fine_row_offset(const uint32_t staged, const uint32_t x, const uint32_t weights = kFineSubWeights)
{
    return fine_udot4((x >> 2) & 0x010101u, weights, staged);
}
// its address where the rows are at rows_at: rows_at + 16 * rank + 2 * sub-cell (a constant rows_at folds into the read)
DP_HD inline uint32_t fine_row_address(const uint32_t staged, const uint32_t x, const uint32_t rows_at)
{
    return fine_row_offset(staged, x) + (rows_at - (uint32_t)kFineSubTag);
}

// ---- the choice of a call: everything above put together, as pure as plan_ordered (host_sanitize.cpp `finechoice`;
// tests/test_ordered_fine_choice_cpu.py) ------------------------------------------------------------------------------------
struct FineTables {  // what the palette has and the call brings (32-bit members: also the record format of the test harness)
    int32_t plain, n_win, n_wide;      // the fine table (fine_pack)
    int32_t sub, sub_win, sub_wide;    // the two-level table (fine_pack_sub)
    int32_t thr_bytes;                 // the padded integer thresholds: th_h * tw_pad * 4
};
struct FineSwitches {  // the product library: {0, kFineKeysShipped, kFineSubShipped}
    int32_t no_fine;   // experiments: DP_NO_FINE_KERNEL
    int32_t keys_cap;  // the highest key level allowed, 0..2 (experiments: DP_FINE_KEYS_MAX)
    int32_t sub_cap;   // the highest SUB level allowed, 0..2 (experiments: DP_FINE_SUB_MAX)
};
struct FineChoice {
    int32_t fine;       // ordered_fine_kernel<1, keys, sub> runs in place of the plan's kernel, on the plan's grid, tile stride and fix-up pass
    int32_t keys, sub;  // (keys is 0 where fine is)
};
// The fine kernel takes over where its table exists and fits (fine_replaces), at the highest key level whose LDS layout fits up
// to the cap, and on the two-level table where the palette has one and it fits at key level 1.  A palette of the product
// library that has the two-level table has the other one only once a call needed it (host.cpp: ensure_fine_table): `sub_only`.
inline FineChoice choose_fine(const OrderedPlan &p, const FineTables &t, const FineSwitches &sw)
{
    const FineFacts f{t.plain, t.n_win, t.n_wide, t.thr_bytes};
    const bool plain = fine_replaces(p, f) && !sw.no_fine;
    const bool sub_only = !t.plain && t.sub && fine_plan_ok(p) && !sw.no_fine;
    const int keys = plain ? std::min(fine_keys_level(f), (int)sw.keys_cap) : (sub_only ? std::min(1, (int)sw.keys_cap) : 0);
    const int sub = fine_sub_level({t.sub && (plain || sub_only), t.sub_win, t.sub_wide, t.thr_bytes, keys, sw.sub_cap});
    const bool fine = plain || sub != 0;
    return {fine, fine ? keys : 0, sub};
}

// The instances of ordered_fine_kernel<1, keys, sub> a build has (ordered.hip: fine_kernel follows this): every (keys, sub) that
// choose_fine can give within the shipped caps, and in the experiments build within any caps.
constexpr bool fine_instance(const int keys, const int sub, const bool experiments)
{
    if (sub == 2) return keys == 1;
    if (sub == 1) return experiments && keys == 1;
    return sub == 0 && (keys == 0 || keys == 1 || (experiments && keys == 2));
}

}  // namespace dp
