// Which ordered-dither kernel serves a call: the decision of launch_ordered (ordered.hip) as a pure function, and the LDS
// budgets that both the decision and the kernels use.  No HIP, no environment: plain C++17 like host_logic.h, included by
// ordered.hip and compiled on its own into the sanitizer harness (host_sanitize.cpp, `orderedplan`), where
// tests/test_ordered_plan_cpu.py compares it case by case with tests/ordered_plan_ref.py.
//
// Order of precedence (plan_ordered), first match wins:
//   integer palette with a cell table that can be staged -- `lean_ok || whole_tab`:
//     1. compact  crowded palettes (`adapt`): the whole octree in LDS, one BYTE per entry, every pixel resolved in place;
//                 two workgroups per CU when table + colours + maps + thresholds fit 80 KB.  Integer thresholds go to LDS
//                 behind the table (MODE 1); a table too large for that -- blue noise -- is read as float32 from L1 (MODE 2).
//     2. fast     uncrowded palettes on plain cells (no warp, no adapt) whose nearest sets were staged (cell_perm): the
//                 nearest set of every cell first, so nearest-only slots read six entries.  It stages the 4096 cell blocks,
//                 the flat lists of the split cells, integer thresholds and two queues.  Measured on MI355X
//                 (profiles/experiments/scripts/fast_vs_lean.py, 24 4K frames, 256 colours): nearest-only mode 0.45 ms
//                 against 0.50 ms of the lean kernel; with a matrix the per-slot class branches cost more than the shorter
//                 candidate network saves (0.66 against 0.55 ms), so the matrix / IGN modes stay on the lean kernel unless
//                 the fast_all switch is set.
//     3. lean     LDS candidate blocks, branch-free main loop, rare pixels (split cells, distance ties, exact equality,
//                 row-straddling groups) deferred to a wave-private queue.  The table it stages: 4-entry blocks when the
//                 accelerator built them (half the candidate work), else 8-entry blocks, or -- crowded palettes -- the
//                 table over warped cells with its maps.  4-entry blocks on plain cells that leave half of LDS free run two
//                 workgroups per CU (HALF).  Crowded palettes (many split cells, or a table larger than LDS) take the
//                 instantiation that adapts per wave (ADAPT).
//                 (Its plainest row -- 8-entry blocks on plain cells, not adaptive, integer thresholds in LDS -- is served by
//                 ordered_fine_kernel where the palette has a fine table: choose_fine (ordered_fine.h) decides that after this
//                 plan, which stays what it was.)
//     4. cell     the previous generation (inline rare paths, the whole plain 8-entry table in dynamic LDS): what is left
//                 for buffers that are not dword-aligned, negative origins and thresholds without a padded copy.
//   float (use_gamma) palette with a cell table, dword-aligned frames:
//     5. compact_float  the one-byte-per-entry table (K <= 256): records + lut + table in LDS
//     6. lean_float     float32 ranking with a certainty gap, float64 recomputation of the winners
//   everything else:
//     7. brute    ordered_int_kernel / ordered_f64_kernel over the whole palette (no accelerator)
// Kept as they were measured, odd as they look: `half` is settled before the family is, so it also sizes the grid of the
// fast and the cell kernel; the compact kernel takes its own grid (comp_half) and the tile stride is worked out again for
// it; the branch is entered on lean_ok but the lean rows test lean_geo and their own threshold condition.
#pragma once
#include <cstdint>

#include "host_logic.h"  // kWideList, kQueueSmall

namespace dp {

// ---- LDS budgets of the ordered kernels (ordered.hip) ------------------------------------------------------------------
constexpr int kBlock = 256;       // brute-force and fix-up kernels
constexpr int kCellBlock = 1024;  // tile kernels: one persistent workgroup walks 4096-pixel tiles
constexpr int kLeanLdsWords = 160 * 1024 / 4;
constexpr int kLeanQueue = 128;                                         // entries per wave
constexpr int kLeanQueueWords = (kCellBlock / 64) * kLeanQueue;         // 8 KB at the top of LDS
constexpr int kLeanTabBytes = (kLeanLdsWords - kLeanQueueWords) * 4;    // table + thresholds must fit below
constexpr int kLeanHalfLdsWords = 80 * 1024 / 4;                        // HALF instances: two workgroups per CU
constexpr int kLeanHalfQueue = 112;                                     // entries per wave: drained from 48 up (47 + 64 at most)
constexpr int kLeanHalfDrain = 48;
constexpr int kLeanHalfTabBytes = (kLeanHalfLdsWords - (kCellBlock / 64) * kLeanHalfQueue) * 4;
constexpr int kWarpLutBytes = 768;                                      // tables over warped cells: the three maps ...
constexpr int kWarpLutAt = kLeanTabBytes - kWarpLutBytes;               // ... sit right below the queue
constexpr int kCompactHalfWords = 80 * 1024 / 4;
constexpr uint32_t kCompactRecBytes = 256 * 8;                           // LDS: records at 0 ...
constexpr uint32_t kCompactLutAt = kCompactRecBytes;                     // ... the three warp maps ...
constexpr uint32_t kCompactTabAt = kCompactLutAt + kWarpLutBytes;        // ... the table, then integer thresholds
constexpr int kFastQueue = 128;  // entries per wave and queue (A and B)
constexpr uint32_t kCfRecBytes = 256 * 16;   // compact_float: records, lut_in, the table
constexpr uint32_t kCfLutAt = kCfRecBytes;
constexpr uint32_t kCfTabAt = kCfLutAt + 256;

// ---- what the decision reads -------------------------------------------------------------------------------------------
// One chunk of frames of one call.  Pointers of PalDev / ThrDev appear as present (1) / absent (0); every member is 32 bits
// wide, so the struct is also the record format of the test harness.
struct OrderedFacts {
    int32_t mode, K, is_integer, n_inner;  // mode: DP_MODE_NEAREST 0, DP_MODE_MATRIX 1, DP_MODE_IGN 2
    uint32_t n_px, hw, w;  // pixels of the chunk, of a frame, of a row
    int32_t y0, x0, aligned;
    int32_t cell_tab, tab_words, tab_total;
    int32_t cell_tab4, tab4_words;
    int32_t warp_tab, warp_words, warp_total, warp_bw, warp_adapt;
    int32_t adapt, cell_perm, cell_perm4, n_wide, n_wide4;
    int32_t comp_tab, comp_words, comp_warp;
    int32_t ftab, ftab_words;
    int32_t m, mpad, fpad, th_h, th_w, tw_pad;  // thresholds as the launch sees them ("none" outside the matrix mode)
    int32_t n_cus;
};

// experiment switches (dp_internal.h: exp_env); all false in the product library
struct OrderedSwitches {
    int32_t lean_no_half, fast_all, force_compact, no_compact_kernel, compact_no_half;
};

enum OrderedFamily { kFamBrute, kFamCell, kFamFast, kFamLean, kFamCompact, kFamLeanFloat, kFamCompactFloat };
enum OrderedTable { kTabPlain8, kTabPlain4, kTabWarped };  // what the lean and fast kernels find in pal.cell_tab / tab_words / tab_total

inline const char *family_name(const OrderedFamily f)
{
    constexpr const char *names[] = {"brute", "cell", "fast", "lean", "compact", "lean_float", "compact_float"};
    return names[f];
}

struct OrderedPlan {
    OrderedFamily family;
    int mode;                    // the kernel's MODE: 0 nearest, 1 matrix in integer form, 2 matrix float32, 3 IGN
    int bw;                      // template arguments of the kernel (lean: all four; fast: bw; compact: warp, half)
    bool adapt, warp, half;
    OrderedTable table;
    uint32_t grid, block;        // pass 1
    uint32_t n_tiles, n_words;   // 4096-pixel tiles (0: brute), words of the flag bitmap
    uint32_t adv_y, adv_x;       // (tile stride of the persistent grid) mod hw, in rows and columns
    uint32_t lds_bytes;          // dynamic LDS (cell kernel only)
    int fix_mode;                // fix-up pass: 0 nearest, 2 matrix (float32 thresholds), 3 IGN
    bool fix_big_queue;          // its traversal queue: kQueueLarge instead of kQueueSmall entries
    uint32_t fix_grid;
};

// what ordered_fast_kernel stages whatever the mode: 4096 cell blocks, the flat lists of the split cells, two queues
constexpr int64_t fast_fixed_bytes(const int bw, const int n_wide)
{
    return 4096 * (int64_t)bw * 4 + (int64_t)n_wide * kWideList * 4 + 2 * (kCellBlock / 64) * kFastQueue * 4;
}

inline OrderedPlan plan_ordered(const OrderedFacts &f, const OrderedSwitches &sw)
{
    constexpr int kNearest = 0, kMatrix = 1, kIgn = 2;
    constexpr int64_t kLdsBytes = 4 * (int64_t)kLeanLdsWords;
    // a single colour: every pixel maps to it, and the k=2 query of the reference has no second entry
    const int mode = f.K == 1 ? kNearest : f.mode;
    const bool integer = f.is_integer != 0;
    const uint32_t groups = (f.n_px + 3) / 4;
    const uint32_t blocks = (groups + kBlock - 1) / kBlock;
    const int64_t thr_bytes = (int64_t)f.th_h * f.tw_pad * 4;

    OrderedPlan p{};
    p.family = kFamBrute;
    p.bw = 8;
    p.table = kTabPlain8;
    p.grid = blocks;
    p.block = kBlock;
    p.n_words = blocks * (kBlock / 64) * 4;
    // MODE of a kernel that takes its integer thresholds when `int_thr`, float32 ones otherwise
    const auto kernel_mode = [mode](const bool int_thr) { return mode == kNearest ? 0 : (mode == kIgn ? 3 : (int_thr ? 1 : 2)); };
    // a persistent grid of `per_cu` workgroups per CU over 4096-pixel tiles, and the stride from a tile to the workgroup's next
    const auto tiles = [&](const uint32_t per_cu) {
        p.n_tiles = (groups + kCellBlock - 1) / kCellBlock;
        p.n_words = p.n_tiles * (kCellBlock / 64) * 4;
        p.block = kCellBlock;
        p.grid = p.n_tiles < (uint32_t)f.n_cus * per_cu ? p.n_tiles : (uint32_t)f.n_cus * per_cu;
        const uint64_t adv = ((uint64_t)p.grid * kCellBlock * 4u) % (uint64_t)f.hw;
        p.adv_y = (uint32_t)(adv / f.w);
        p.adv_x = (uint32_t)(adv % f.w);
    };

    const bool int_thr_ok = f.m != 0 && f.th_h * f.th_w <= 256;  // ordered_int_kernel / ordered_cell_kernel keep 256 in LDS
    const bool warp = f.warp_tab != 0;
    const bool small = warp ? f.warp_bw == 4 : f.cell_tab4 != 0;
    const int64_t lean_tab_bytes = warp ? 4 * (int64_t)f.warp_words + kWarpLutBytes : 4 * (int64_t)(small ? f.tab4_words : f.tab_words);
    const bool origin_ok = f.aligned != 0 && f.y0 >= 0 && f.x0 >= 0;
    const bool geo_ok = integer && (warp || small || f.cell_tab != 0) && origin_ok && f.n_px <= (1u << 30);
    const bool lean_geo = geo_ok && lean_tab_bytes <= kLeanTabBytes;
    const bool int_lean = f.mpad != 0 && lean_tab_bytes + thr_bytes <= kLeanTabBytes;
    // (every tile kernel but the cell kernel: the matrix mode needs integer thresholds that fit its LDS, or the padded float32 rows)
    const auto mode_ok = [&](const bool int_thr) { return mode == kNearest || mode == kIgn || (mode == kMatrix && (int_thr || f.fpad != 0)); };
    const bool lean_ok = lean_geo && mode_ok(int_lean);
    const bool whole_tab = f.cell_tab != 0 && f.tab_total == f.tab_words;  // the cell kernel stages all of it

    if (integer && (lean_ok || whole_tab)) {
        const bool half = lean_ok && small && !warp && !sw.lean_no_half &&
                          lean_tab_bytes + (mode == kMatrix && int_lean ? thr_bytes : 0) <= kLeanHalfTabBytes;
        tiles(half ? 2u : 1u);
        const OrderedTable table = warp ? kTabWarped : (small ? kTabPlain4 : kTabPlain8);
        const bool adapt = warp ? f.warp_adapt != 0 : (!small && f.adapt != 0);
        const int64_t fast_fixed = fast_fixed_bytes(small ? 4 : 8, small ? f.n_wide4 : f.n_wide);
        const bool int_fast = f.mpad != 0 && fast_fixed + thr_bytes <= kLdsBytes;
        const bool fast_ok = (mode == kNearest || sw.fast_all) && geo_ok && !warp && !adapt && (small ? f.cell_perm4 : f.cell_perm) != 0 &&
                             fast_fixed <= kLdsBytes && mode_ok(int_fast);
        const int64_t comp_base = f.comp_tab ? (int64_t)kCompactTabAt + 4 * (int64_t)f.comp_words : 0;
        const bool int_comp = mode == kMatrix && f.mpad != 0 && comp_base + thr_bytes <= kLdsBytes;
        const int64_t comp_bytes = comp_base + (int_comp ? thr_bytes : 0);
        const bool comp_ok = f.comp_tab != 0 && geo_ok && (adapt || sw.force_compact) && comp_bytes <= kLdsBytes && mode_ok(int_comp) &&
                             !sw.no_compact_kernel;
        if (comp_ok) {
            p.family = kFamCompact;
            p.mode = kernel_mode(int_comp);
            p.warp = f.comp_warp != 0;
            p.half = comp_bytes <= 4 * (int64_t)kCompactHalfWords && !sw.compact_no_half;
            tiles(p.half ? 2u : 1u);
        } else if (fast_ok) {
            p.family = kFamFast;
            p.mode = kernel_mode(int_fast);
            p.bw = small ? 4 : 8;
            p.table = table;
        } else if (lean_geo && mode_ok(int_lean)) {
            p.family = kFamLean;
            p.mode = kernel_mode(int_lean);
            p.table = table;
            p.warp = warp;
            p.bw = small ? 4 : 8;
            p.adapt = !small && adapt;  // (a warped table of 4-entry blocks has no adaptive instantiation)
            p.half = !warp && small && half;
        } else {
            p.family = kFamCell;
            p.mode = kernel_mode(int_thr_ok);
            p.lds_bytes = (uint32_t)(sizeof(uint32_t) * ((size_t)f.tab_words + 256));
        }
    } else if (!integer && f.ftab != 0 && origin_ok && (int64_t)f.ftab_words * 4 + (int64_t)f.K * 16 + 256 <= kLdsBytes &&  // staged part
               (mode != kMatrix || f.fpad != 0)) {
        const int64_t cf_bytes = f.comp_tab ? (int64_t)kCfTabAt + 4 * (int64_t)f.comp_words : 0;
        const bool cf_ok = f.comp_tab != 0 && cf_bytes <= kLdsBytes && !sw.no_compact_kernel;
        p.family = cf_ok ? kFamCompactFloat : kFamLeanFloat;
        p.mode = kernel_mode(false);
        tiles(1u);
    } else {
        p.mode = kernel_mode(integer && int_thr_ok);
    }
    p.fix_mode = p.mode == 1 ? 2 : p.mode;
    p.fix_big_queue = f.n_inner > kQueueSmall;
    // one resident workgroup per CU (the 96 KB LDS list admits no more): a persistent grid avoids queueing
    const uint32_t fix_blocks = (p.n_words + kBlock * 8 - 1) / (kBlock * 8);
    p.fix_grid = fix_blocks < (uint32_t)f.n_cus ? fix_blocks : (uint32_t)f.n_cus;
    return p;
}

}  // namespace dp
