// CPU-sanitizer harness for the host logic of libditherpie_hip.so (host_logic.h, ed_tables.h): built WITHOUT HIP by
//   make host_asan   ->  build/host_asan   (g++ -fsanitize=address,undefined)
//   make host_tsan   ->  build/host_tsan   (g++ -fsanitize=thread: the multi-threaded per-cell loops)
// and run by tests/test_host_sanitizers.py in the CPU tier.  Test infrastructure, not part of the product library.
//
//   host_xxx kdtree   <pts.f64> <K>   the scipy-order KD-tree build; prints indices / nodes / splits (compared with
//                                     the golden cKDTree structures by the test)
//   host_xxx edtables <pts.f64> <K>   the diffusion candidate tables (ed_tables.h) from host-made geometric lists (the criterion of
//                                     ed_cells_kernel), then checks on sampled points that the true nearest entry (and
//                                     everything tied with it) is on the list the kernels would search
//   host_xxx edtablesdigest <pts.f64> <K> <what>   the same tables (what: 1 = ed_tables_build, 2 = ed_ext_build, 3 = both) without
//                                     any check: prints size and CRC-32 of every table's bytes on one line (compared with
//                                     tests/golden/ed_tables_digests.json, which pins the tables' bytes)
//   host_xxx accel    <pts.f64> <K> <bw>   the accelerator's cell table from brute-force membership masks (what
//                                     accel_scan_kernel computes on the device), nearest sets, staging orders, wide
//                                     lists, node reordering, warp maps; checks on sampled colours that the block a
//                                     kernel would reach holds all of T(x)
//   host_xxx mediancut <rgb.u8> <n> <depth>   the replay of CPython's set order + the counting-sort median cut; prints the
//                                     palette and the first 2000 entries of the order (compared with the interpreter's own
//                                     set and with the Python cut by the test)
//   host_xxx indexmap <lists.bin> <n>   the colour -> index hash tables of the indexed output (index_map_build): the file holds
//                                     n records {int32 K, int32 Q, K x 3 colour bytes, Q x 3 query bytes}; per record prints
//                                     the map's figures, the index index_map_lookup reports for each of the K colours
//                                     and how many of the Q queries (absent colours, by the test's construction) it finds
//   host_xxx giflzw <cases.bin> <n>   the host statement of the GIF image data (gif_lzw_encode): the file holds n records
//                                     {int32 n_frames, h, w, min_code_size; int64 chunk_px; n_frames x h x w index bytes}; per
//                                     frame prints its size and its bytes in hex (compared with tests/gif_ref.py by the test)
//   host_xxx pngdeflate <cases.bin> <n>   the host statement of the PNG-8 image data (png_deflate_encode): n records of
//                                     int32 frames, h, w, depth, seg_bytes and frames * h * w index bytes; every frame prints
//                                     its size and its zlib stream in hex (inflated and compared by the test)
//   host_xxx pngfile <cases.bin> <n>   the host statements of the finished chunks and their CRCs (png_file_assemble, crc32_bytes,
//                                      crc32_combine): n records of 8 int32 (frames, stride, n_idat, seq0, seq_step, pre_bytes,
//                                      per-frame prefixes 0 / 1, post_bytes), the int64 sizes, the streams, the prefixes, the suffix
//   host_xxx pngdyn <cases.bin> <n>   the same with dynamic-Huffman blocks as a third candidate (png_deflate_encode_dyn)
//   host_xxx orderedplan <cases.bin> <n>   the kernel choice of the ordered dither (ordered_plan.h: plan_ordered): n records of
//                                     one OrderedFacts and one OrderedSwitches (int32 fields in declaration order); prints one
//                                     plan per line (compared with tests/ordered_plan_ref.py by the test)
//   host_xxx finepack <pal.u8> <K> <out.bin>   the fine table of the ordered dither (host_logic.h: fine_pack) from brute-force
//                                     sets N and T of the 32^3 cells (what accel_scan_kernel computes on the device) within the
//                                     budget of ordered_fine.h; writes int32 ok, n_win, n_wide, image words, then off, the windows
//                                     and the wide lists as palette indices (uint16), then quads, pairs, lists and the LDS image
//                                     (uint32) for tests/test_ordered_fine_cpu.py to check against numpy
//   host_xxx fineplan <cases.bin> <n>   whether the fine kernel replaces a plan (ordered_fine.h: fine_replaces): n records of one
//                                     OrderedFacts, one OrderedSwitches and one FineFacts; prints 0 / 1 per line
//   host_xxx finekeys <cases.bin> <n>   the key level of the fine kernel (ordered_fine.h: fine_keys_level): n records of one FineFacts;
//                                     prints one level per line
//   host_xxx finesub <pal.u8> <K> <out.bin>   the two-level fine table (host_logic.h: fine_pack_sub) from the same brute-force sets,
//                                     packed twice (the same answer) within fine_sub_fits, every sub-cell's window checked against
//                                     sets brute-forced over the whole palette; writes int32 ok, n_win, n_wide, still-wide sub-cells,
//                                     image words, then (uint16) off with its tags, the rows, the windows as palette indices, the wide
//                                     cells, the still-wide sub-cells (8 * rank + sub-cell), the flat lists as palette indices, then
//                                     (uint32) quads, pairs, lists as colours and the image, for tests/test_ordered_fine_sub_cpu.py
//   host_xxx finesublevel <cases.bin> <n>   the SUB level of a call (ordered_fine.h: fine_sub_level): n records of one FineSubFacts;
//                                     prints one level per line
//   host_xxx finechoice <cases.bin> <n>   the fine kernel of a call (ordered_fine.h: choose_fine after plan_ordered): n records of one
//                                     OrderedFacts, one OrderedSwitches, one FineTables and one FineSwitches; prints the plan's family,
//                                     fine, keys, sub, and whether the product and the experiments build have that instance (fine_instance)
//   host_xxx fineaddr <first> <n>     the address arithmetic of the fine kernel's main loop (ordered_fine.h) on the n colours from
//                                     `first` on (0 16777216: all of them): fine_cell_offset against 2 * fine_cell, with and without a
//                                     base and with garbage in bits 24-31; then, whatever the range, every rank and sub-cell:
//                                     fine_stage_tag / fine_stage_tags2 / fine_tag_rank and fine_row_address against rows_at + 16 * rank
//                                     + 2 * sub-cell on the 64 colours of the sub-cell; prints the counts and the number of mismatches
//   host_xxx fixneeded <cases.bin> <n>   whether a call keeps its fix-up pass (ordered_fix.h: fix_needed): n records of one FixFacts and
//                                     one FixSwitches; prints 0 / 1 per line (compared with tests/ordered_fix_ref.py by the test)
// Exit code 0 = all checks passed (and the sanitizer had nothing to say).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host_logic.h"
#include "ordered_plan.h"
#include "ordered_fine.h"
#include "ordered_fix.h"

using namespace dp;

static std::vector<double> read_pts(const char *path, int K)
{
    std::vector<double> p((size_t)K * 3);
    FILE *f = fopen(path, "rb");
    if (!f || fread(p.data(), sizeof(double), p.size(), f) != p.size()) {
        fprintf(stderr, "cannot read %d points from %s\n", K, path);
        exit(2);
    }
    fclose(f);
    return p;
}

static uint32_t lcg(uint32_t &s)
{
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

static int run_kdtree(const std::vector<double> &pts, int K)
{
    HostTree t;
    build_tree(pts.data(), K, t);
    printf("indices");
    for (int v : t.indices) printf(" %d", v);
    printf("\nnodes %zu\n", t.split_dim.size());
    for (size_t i = 0; i < t.split_dim.size(); ++i)
        printf("%d %d %d %d %d %.17g\n", t.split_dim[i], t.start[i], t.end[i], t.less[i], t.greater[i], t.split[i]);
    printf("box %.17g %.17g %.17g %.17g %.17g %.17g\n", t.mins[0], t.mins[1], t.mins[2], t.maxes[0], t.maxes[1], t.maxes[2]);
    return 0;
}

// ---- diffusion tables ----------------------------------------------------------------------------------------------
static void geometric_list(const std::vector<double> &pts, int K, const double lo[3], double size, std::vector<int> &list)
{
    double bound = std::numeric_limits<double>::infinity();
    for (int j = 0; j < K; ++j) {
        double far2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double c = pts[3 * j + k], m = std::max(std::fabs(c - lo[k]), std::fabs(c - (lo[k] + size)));
            far2 += m * m;
        }
        bound = std::min(bound, far2);
    }
    bound = bound * (1.0 + 1e-6) + 1e-3;  // (the kernel works in float32 with a slack)
    list.clear();
    for (int j = 0; j < K; ++j) {
        double near2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double c = pts[3 * j + k], m = std::max(std::max(lo[k] - c, c - (lo[k] + size)), 0.0);
            near2 += m * m;
        }
        if (near2 <= bound) list.push_back(j);
    }
}

static bool listed(const U4 &e, int n_max, int j, bool wide = false)
{
    const uint32_t w[4] = {e.x, e.y, e.z, e.w};
    const int n = (int)(w[0] & 255u);
    if (n > n_max) return true;  // overflow marker: the kernel scans the palette
    for (int i = 1; i <= n; ++i)
        if (ed_list_get(w, i - 1, wide) == j) return true;
    return false;
}

// the 8^3 lists as ed_cells_kernel leaves them: the geometric criterion, count 255 where a list is longer than the format holds
static std::vector<U4> geometric_cells(const std::vector<double> &pts, int K)
{
    const bool wide = K > 256;   // ten-bit list entries (ed_tables.h: ed_list_put)
    const int cap = ed_list_cap(K);
    std::vector<U4> cells(kEdCells);
    std::vector<int> list;
    for (int cell = 0; cell < kEdCells; ++cell) {
        const double lo[3] = {(double)((cell & 31) * 8), (double)(((cell >> 5) & 31) * 8), (double)((cell >> 10) * 8)};
        geometric_list(pts, K, lo, 8.0, list);
        uint32_t w[4] = {255u, 0u, 0u, 0u};
        if ((int)list.size() <= cap) {
            w[0] = (uint32_t)list.size();
            for (size_t n = 1; n <= list.size(); ++n) ed_list_put(w, (int)n - 1, list[n - 1], wide);
        }
        cells[cell] = make_u4(w[0], w[1], w[2], w[3]);
    }
    return cells;
}

// what: 1 = the tables every diffusion kernel uses, 2 = the extended lists of the unclamped diffusers, 3 = both
static void build_edtables(const std::vector<double> &pts, int K, int what, std::vector<U4> &cells, EdTables &tb)
{
    const EdPalette pal = ed_palette(pts.data(), K);
    if (what & 1) ed_tables_build(pal, cells, tb);
    if (what & 2) ed_ext_build(pal, tb);
}

// No self-check: size and CRC-32 of every table's bytes on one line, for tests/golden/ed_tables_digests.json.
static int run_edtablesdigest(const std::vector<double> &pts, int K, int what)
{
    if (K < 9 || K > 1024 || what < 1 || what > 3) {
        fprintf(stderr, "edtablesdigest: 9 <= K <= 1024, what 1, 2 or 3\n");
        return 2;
    }
    std::vector<U4> cells = geometric_cells(pts, K);
    EdTables tb;
    build_edtables(pts, K, what, cells, tb);
    auto digest = [](const char *name, const void *p, const size_t n, const size_t elem) {
        printf(" %s=%zu:%08x", name, n, crc32_bytes(static_cast<const uint8_t *>(p), n * elem));
    };
    printf("edtablesdigest K=%d what=%d", K, what);
    digest("cells", cells.data(), cells.size(), sizeof(U4));
    digest("nodes", tb.nodes.data(), tb.nodes.size(), sizeof(U4));
    digest("l16", tb.l16.data(), tb.l16.size(), sizeof(U4));
    digest("coarse", tb.coarse.data(), tb.coarse.size(), sizeof(uint32_t));
    digest("ext", tb.ext.data(), tb.ext.size(), sizeof(uint32_t));
    digest("ext16", tb.ext16.data(), tb.ext16.size(), sizeof(U4));
    digest("ext_nodes", tb.ext_nodes.data(), tb.ext_nodes.size(), sizeof(U4));
    digest("h4", tb.h4.data(), tb.h4.size(), sizeof(uint32_t));
    printf(" h4_wanted=%zu h4_depth=%.17g h4_none=%.17g\n", tb.h4_wanted, tb.h4_depth, tb.h4_none);
    return 0;
}

static int run_edtables(const std::vector<double> &pts, int K)
{
    if (K < 9 || K > 1024) {
        fprintf(stderr, "edtables: 9 <= K <= 1024\n");
        return 2;
    }
    const bool wide = K > 256;   // ten-bit list entries (ed_tables.h: ed_list_put)
    const int cap = ed_list_cap(K);
    std::vector<U4> cells = geometric_cells(pts, K);
    EdTables tb;
    build_edtables(pts, K, 3, cells, tb);   // (the diffusion tables AND the extended lists of the unclamped diffusers)
    // sampled points: uniform integers, the palette entries themselves (rounded) and their neighbours
    uint32_t seed = 12345u + (uint32_t)K;
    long checked = 0, bad = 0, h4_answers = 0, h4_none = 0;
    auto check_point = [&](const int x[3]) {
        double best = std::numeric_limits<double>::infinity();
        for (int j = 0; j < K; ++j) {
            double d = 0;
            for (int k = 0; k < 3; ++k) d += (x[k] - pts[3 * j + k]) * (x[k] - pts[3 * j + k]);
            best = std::min(best, d);
        }
        // walk: 8^3 cell -> nodes
        U4 e = cells[(x[0] >> 3) | ((x[1] >> 3) << 5) | ((x[2] >> 3) << 10)];
        double lo[3] = {(double)(x[0] & ~7), (double)(x[1] & ~7), (double)(x[2] & ~7)}, size = 8.0;
        while ((e.x & 255u) == 254u) {
            const size_t node = e.x >> 8;
            size *= 0.5;
            int sub = 0;
            for (int k = 0; k < 3; ++k)
                if (x[k] >= lo[k] + size) {
                    sub |= 1 << k;
                    lo[k] += size;
                }
            if (node * 8 + sub >= tb.nodes.size()) {
                ++bad;
                return;
            }
            e = tb.nodes[node * 8 + sub];
        }
        const int c16 = (x[0] >> 4) | ((x[1] >> 4) << 4) | ((x[2] >> 4) << 8);
        for (int j = 0; j < K; ++j) {
            double d = 0;
            for (int k = 0; k < 3; ++k) d += (x[k] - pts[3 * j + k]) * (x[k] - pts[3 * j + k]);
            if (d != best) continue;
            ++checked;
            if (!listed(e, cap, j, wide)) ++bad;
            if (!tb.l16.empty() && !listed(tb.l16[c16], cap, j, wide)) ++bad;
            if (!tb.h4.empty()) {
                // the hierarchical <= 4-entry table as nearest_h4 (ed_nearest.hip.h) walks it: a leaf must hold every nearest entry
                auto marker = [](const uint32_t w) { return (w & 0xffu) >= ((w >> 8) & 0xffu); };
                uint32_t w = tb.h4[c16];
                bool answer = true;
                for (int bit = 3; bit >= 1 && marker(w); --bit) {
                    if ((w >> 16) == 0xffffu) {
                        answer = false;
                        break;
                    }
                    const size_t at = 4096u + (size_t)(w >> 16) * 8u + (size_t)(((x[0] >> bit) & 1) | (((x[1] >> bit) & 1) << 1) | (((x[2] >> bit) & 1) << 2));
                    if (at >= tb.h4.size()) {
                        ++bad;
                        answer = false;
                        break;
                    }
                    w = tb.h4[at];
                }
                if (answer && marker(w)) answer = false;   // (still a node pointer below 2-wide: no answer, the lists decide)
                if (answer) {
                    ++h4_answers;
                    bool on_leaf = false;
                    for (int b = 0; b < 4; ++b) on_leaf |= (int)((w >> (8 * b)) & 255u) == j;
                    if (!on_leaf) ++bad;
                } else {
                    ++h4_none;
                }
            }
            for (const std::vector<uint32_t> *tab : {&tb.coarse, &tb.ext}) {
                if (tab->empty()) continue;
                const uint32_t word = (*tab)[c16];
                const int n = (int)(word & 15u);
                bool ok = n > 7;
                for (int i = 0; i < n && !ok; ++i) ok = (int)((word >> (4 * (i + 1))) & 15u) == j;
                if (!ok) ++bad;
            }
        }
    };
    for (int i = 0; i < 40000; ++i) {
        const int x[3] = {(int)(lcg(seed) & 255u), (int)(lcg(seed) & 255u), (int)(lcg(seed) & 255u)};
        check_point(x);
    }
    for (int j = 0; j < K; ++j)
        for (int d = -1; d <= 1; ++d) {
            int x[3];
            for (int k = 0; k < 3; ++k) x[k] = std::min(255, std::max(0, (int)std::lround(pts[3 * j + k]) + d));
            check_point(x);
        }
    // the extended 16^3 lists (17..256 colours, unclamped diffusers): points in and around the cube, looked up by their clamped cell
    long ext_checked = 0, ext_long = 0;
    if (!tb.ext16.empty()) {
        for (int i = 0; i < 60000; ++i) {
            double x[3];
            for (int k = 0; k < 3; ++k) x[k] = (double)((int)(lcg(seed) % 640u) - 192) + (double)(lcg(seed) & 255u) / 256.0;   // [-192, 448)
            double best = std::numeric_limits<double>::infinity();
            for (int j = 0; j < K; ++j) {
                double d = 0;
                for (int k = 0; k < 3; ++k) d += (x[k] - pts[3 * j + k]) * (x[k] - pts[3 * j + k]);
                best = std::min(best, d);
            }
            int c[3];
            for (int k = 0; k < 3; ++k) c[k] = std::min(15, std::max(0, (int)x[k] >> 4));   // as nearest_ext16 (vardiff.hip)
            U4 e = tb.ext16[(size_t)(c[0] | (c[1] << 4) | (c[2] << 8))];
            int xi[3];
            for (int k = 0; k < 3; ++k) xi[k] = std::min(255, std::max(0, (int)x[k]));   // clamped integer coordinates choose the children
            for (int bit = 3; (e.x & 255u) == 254u; --bit) {
                const size_t at = (size_t)(e.x >> 8) * 8 + (size_t)(((xi[0] >> bit) & 1) | (((xi[1] >> bit) & 1) << 1) | (((xi[2] >> bit) & 1) << 2));
                if (bit < 0 || at >= tb.ext_nodes.size()) {
                    ++bad;
                    break;
                }
                e = tb.ext_nodes[at];
            }
            if ((e.x & 255u) == 254u) continue;
            if ((int)(e.x & 255u) > cap) {
                ++ext_long;
                continue;
            }
            for (int j = 0; j < K; ++j) {
                double d = 0;
                for (int k = 0; k < 3; ++k) d += (x[k] - pts[3 * j + k]) * (x[k] - pts[3 * j + k]);
                if (d != best) continue;
                ++ext_checked;
                if (!listed(e, cap, j, wide)) ++bad;
            }
        }
    }
    printf("ext16=%zu nodes=%zu (checked %ld, in cells with long lists %ld) ", tb.ext16.size(), tb.ext_nodes.size() / 8, ext_checked, ext_long);
    printf("edtables K=%d nodes=%zu l16=%zu coarse=%zu ext=%zu h4=%zu (answers %ld, none %ld) checked=%ld bad=%ld\n", K, tb.nodes.size(),
           tb.l16.size(), tb.coarse.size(), tb.ext.size(), tb.h4.size(), h4_answers, h4_none, checked, bad);
    if (K > 16 && !tb.h4.empty() && h4_answers < 100 * std::max(h4_none, 1L)) return 1;   // the table must answer nearly always
    return bad ? 1 : 0;
}

// ---- accelerator table -----------------------------------------------------------------------------------------------
static int run_accel(const std::vector<double> &pts, int K, int bw)
{
    if (K < 2 || K > 64 || (bw != 4 && bw != 8)) {
        fprintf(stderr, "accel: 2 <= K <= 64 (the masks are brute-forced over 2^24 colours), bw 4 or 8\n");
        return 2;
    }
    const int mw = (K + 31) / 32;
    std::vector<int> pr(K), pg(K), pb(K);
    std::vector<uint32_t> coord4(K);
    for (int j = 0; j < K; ++j) {
        pr[j] = (int)pts[3 * j], pg[j] = (int)pts[3 * j + 1], pb[j] = (int)pts[3 * j + 2];
        coord4[j] = (uint32_t)pr[j] | ((uint32_t)pg[j] << 8) | ((uint32_t)pb[j] << 16);
    }
    // T(x) = everything at least as close as the second nearest; N(x) = the nearest set
    auto sets_of = [&](int r, int g, int b, uint32_t *tm, uint32_t *nm) {
        int d[64], d0 = 1 << 30, d1 = 1 << 30;
        for (int j = 0; j < K; ++j) {
            d[j] = (r - pr[j]) * (r - pr[j]) + (g - pg[j]) * (g - pg[j]) + (b - pb[j]) * (b - pb[j]);
            if (d[j] < d0) {
                d1 = d0;
                d0 = d[j];
            } else if (d[j] < d1) {
                d1 = d[j];
            }
        }
        for (int j = 0; j < K; ++j) {
            if (d[j] <= d1) tm[j >> 5] |= 1u << (j & 31);
            if (nm && d[j] == d0) nm[j >> 5] |= 1u << (j & 31);
        }
    };
    constexpr int kNCells = 4096;
    std::vector<uint32_t> masks((size_t)kNCells * 9 * mw, 0u), nmasks((size_t)kNCells * mw, 0u);
    for (int r = 0; r < 256; ++r)
        for (int g = 0; g < 256; ++g)
            for (int b = 0; b < 256; ++b) {
                const int cell = ((r >> 4) << 8) | ((g >> 4) << 4) | (b >> 4);
                const int sidx = (((r >> 3) & 1) << 2) | (((g >> 3) & 1) << 1) | ((b >> 3) & 1);
                uint32_t tm[2] = {0, 0};
                sets_of(r, g, b, tm, &nmasks[(size_t)cell * mw]);
                for (int w = 0; w < mw; ++w) {
                    masks[((size_t)cell * 9) * mw + w] |= tm[w];
                    masks[((size_t)cell * 9 + 1 + sidx) * mw + w] |= tm[w];
                }
            }
    auto box_masks = [&](const std::vector<Box> &boxes, std::vector<uint32_t> &bm) {
        std::fill(bm.begin(), bm.end(), 0u);
        for (size_t q = 0; q < boxes.size(); ++q)
            for (int r = boxes[q].r0; r < boxes[q].r0 + boxes[q].size; ++r)
                for (int g = boxes[q].g0; g < boxes[q].g0 + boxes[q].size; ++g)
                    for (int b = boxes[q].b0; b < boxes[q].b0 + boxes[q].size; ++b) sets_of(r, g, b, &bm[q * (size_t)mw], nullptr);
        return (int)DP_OK;
    };
    std::vector<uint32_t> tab, perm, wide;
    TableStats st;
    int rc = assemble_table(masks, mw, bw, kTabMaxWords, K, coord4, coord4, box_masks, tab, st, nmasks.data(), bw == 8 ? kNearSlots : 4,
                            &perm, &wide);
    if (rc != DP_OK || st.too_big) {
        fprintf(stderr, "assemble_table failed (rc %d, too_big %d)\n", rc, (int)st.too_big);
        return 1;
    }
    crowded_nodes_first(tab, st, bw, coord4);
    WarpMaps wm;
    make_warp(coord4, wm);
    const std::vector<uint32_t> mp = mass_points(coord4);
    const int in_split = entries_in_split_cells(tab, bw, mp);
    // every sampled colour must find all of T(x) in the block the kernel reaches
    uint32_t seed = 777u + (uint32_t)K;
    long bad = 0, checked = 0;
    for (int i = 0; i < 60000 + 27 * K; ++i) {
        int r, g, b;
        if (i < 60000) {
            r = lcg(seed) & 255, g = lcg(seed) & 255, b = lcg(seed) & 255;
        } else {
            const int q = i - 60000, j = q / 27, o = q % 27;
            r = std::min(255, std::max(0, pr[j] + o % 3 - 1));
            g = std::min(255, std::max(0, pg[j] + (o / 3) % 3 - 1));
            b = std::min(255, std::max(0, pb[j] + o / 9 - 1));
        }
        uint32_t tm[2] = {0, 0};
        sets_of(r, g, b, tm, nullptr);
        size_t pos = (size_t)cell_slot(r >> 4, g >> 4, b >> 4) * bw;
        int size = 16, r0 = r & ~15, g0 = g & ~15, b0 = b & ~15;
        bool slow = false;
        while (tab[pos] >> 31) {
            if ((tab[pos] >> 30) == 3u) {
                slow = true;  // a single colour with more candidates than a block: the fix-up pass resolves it
                break;
            }
            const size_t node = tab[pos] & 0xffffffu;
            size /= 2;
            const int sidx = ((r >= r0 + size) << 2) | ((g >= g0 + size) << 1) | (b >= b0 + size);
            r0 += (r >= r0 + size) * size, g0 += (g >= g0 + size) * size, b0 += (b >= b0 + size) * size;
            pos = (size_t)kCells * bw + (node * 8 + sidx) * bw;
            if (pos + bw > tab.size()) {
                ++bad;
                slow = true;
                break;
            }
        }
        if (slow) continue;
        for (int j = 0; j < K; ++j)
            if (tm[j >> 5] >> (j & 31) & 1u) {
                ++checked;
                bool found = false;
                for (int e = 0; e < bw; ++e) found |= tab[pos + e] == coord4[j];
                bad += !found;
            }
    }
    // the fast kernel's staging orders: a permutation of the block's positions, nearest set first
    for (int slot = 0; slot < kCells; ++slot) {
        const uint32_t pw = perm[slot];
        if (pw == 0xffffffffu) continue;
        if ((pw >> 24) == 0xffu) {
            if (((size_t)(pw & 0xffffffu) + 1) * kWideList > wide.size()) ++bad;
            continue;
        }
        const int fb = bw == 8 ? 3 : 2;
        uint32_t seen = 0;
        for (int k = 0; k < bw; ++k) seen |= 1u << ((pw >> (fb * k)) & ((1u << fb) - 1));
        if (seen != (1u << bw) - 1u) ++bad;
    }
    // the one-byte-per-entry copy (ordered_compact_kernel): same blocks, same positions, markers as byte offsets of the node
    int compact_bad = 0;
    if (bw == 8) {
        const std::vector<uint32_t> ct = compact_table(tab, coord4);
        compact_bad += ct.size() * 4 != tab.size();
        for (size_t b = 0; b + 8 <= tab.size(); b += 8) {
            const uint32_t lo = ct[b / 4], hi = ct[b / 4 + 1];
            if (tab[b] >> 31) {
                compact_bad += hi != 0xffffffffu;
                if ((tab[b] >> 30) == 2u) {
                    const uint32_t off = lo & 0xffffffu;  // bytes from the start of the compact table
                    compact_bad += (lo >> 30) != 2u || off != (4096u + (tab[b] & 0xffffffu) * 8u) * 8u || off + 64u > ct.size() * 4u;
                } else {
                    compact_bad += lo != 0xC0000000u;
                }
                continue;
            }
            uint32_t prev = 0;
            for (int i = 0; i < 8; ++i) {
                const uint32_t idx = ((i < 4 ? lo : hi) >> (8 * (i & 3))) & 255u;
                compact_bad += idx >= (uint32_t)K || coord4[idx] != tab[b + i];
                compact_bad += i > 0 && idx <= prev && coord4[idx] != coord4[prev];  // index order (equal colours: ascending too)
                prev = idx;
            }
        }
    }
    int warp_bad = 0;
    for (int c = 0; c < 3; ++c)
        for (int x = 1; x < 256; ++x) warp_bad += wm.lut[c][x] < wm.lut[c][x - 1];
    printf("accel K=%d bw=%d words=%zu split=%d split_cells=%d slow=%d max_cnt=%d wide=%zu mass_in_split=%d/%zu checked=%ld bad=%ld warp_bad=%d compact_bad=%d\n",
           K, bw, tab.size(), st.n_split, st.n_split_cells, st.n_slow, st.max_cnt, wide.size() / kWideList, in_split, mp.size(),
           checked, bad, warp_bad, compact_bad);
    return (bad || warp_bad || compact_bad) ? 1 : 0;
}

// ---- median cut (set-order replay + counting-sort cut) ----------------------------------------------------------------
static int run_mediancut(const char *path, long n, int depth)
{
    std::vector<uint8_t> rgb((size_t)n * 3 + 1);
    FILE *f = fopen(path, "rb");
    if (!f || fread(rgb.data(), 3, (size_t)n, f) != (size_t)n) {
        fprintf(stderr, "cannot read %ld colours from %s\n", n, path);
        return 2;
    }
    fclose(f);
    std::vector<uint32_t> order;
    pyset_order(rgb.data(), (size_t)n, order);
    std::vector<uint32_t> colours(order.size() + 1), scratch(order.size() + 1);
    for (size_t i = 0; i < order.size(); ++i) {
        const uint8_t *c = rgb.data() + 3 * (size_t)order[i];
        colours[i] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    }
    std::vector<int32_t> out;
    median_cut_u32(colours.data(), scratch.data(), order.size(), depth, out, 8);
    printf("distinct %zu\npalette", order.size());
    for (int32_t v : out) printf(" %d", v);
    printf("\norder");
    for (size_t i = 0; i < order.size() && i < 2000; ++i) printf(" %u", order[i]);
    printf("\n");
    return 0;
}

// ---- index maps ----------------------------------------------------------------------------------------------------
static int run_indexmap(const char *path, const int n_lists)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int l = 0; l < n_lists; ++l) {
        int32_t head[2];
        if (fread(head, sizeof(int32_t), 2, f) != 2 || head[0] < 1 || head[0] > DP_MAX_COLORS || head[1] < 0) {
            fprintf(stderr, "bad record %d in %s\n", l, path);
            return 2;
        }
        const int K = head[0], Q = head[1];
        std::vector<uint8_t> colours((size_t)K * 3), queries((size_t)Q * 3 + 1);
        if (fread(colours.data(), 3, (size_t)K, f) != (size_t)K || fread(queries.data(), 3, (size_t)Q, f) != (size_t)Q) {
            fprintf(stderr, "short record %d in %s\n", l, path);
            return 2;
        }
        IndexMapHost m;
        if (!index_map_build(colours.data(), K, m)) {
            printf("map %d K=%d failed\n", l, K);
            continue;
        }
        int used = 0;
        for (uint32_t w : m.table) used += w != kIndexMapEmpty;
        printf("map %d K=%d slots=%d rest_bits=%d max_probe=%d bound=%d mult=%u used=%d\nidx", l, K, m.slots, m.rest_bits, m.max_probe,
               kIndexMapMaxProbe, m.mult, used);
        for (int j = 0; j < K; ++j) printf(" %d", index_map_lookup(m, m.colors[(size_t)j]));
        int hits = 0;
        for (int q = 0; q < Q; ++q) {
            const uint8_t *c = queries.data() + 3 * (size_t)q;
            hits += index_map_lookup(m, (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16)) >= 0;
        }
        printf("\nabsent_hits=%d of %d\n", hits, Q);
    }
    fclose(f);
    return 0;
}

// ---- GIF image data --------------------------------------------------------------------------------------------
static int run_giflzw(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[4];
        int64_t chunk = 0;
        if (fread(head, sizeof(int32_t), 4, f) != 4 || fread(&chunk, sizeof(int64_t), 1, f) != 1 || head[0] < 0 || head[1] < 1 || head[2] < 1 ||
            head[3] < 2 || head[3] > 8 || chunk < 1) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const size_t n_px = (size_t)head[1] * (size_t)head[2];
        std::vector<uint8_t> plane(n_px), out;   // exactly n_px bytes: a read past the plane is a sanitizer report
        const uint64_t bound = gif_lzw_bound((int64_t)n_px, chunk);
        for (int k = 0; k < head[0]; ++k) {
            if (fread(plane.data(), 1, n_px, f) != n_px) {
                fprintf(stderr, "short record %d in %s\n", c, path);
                return 2;
            }
            gif_lzw_encode(plane.data(), (int64_t)n_px, head[3], chunk, out);
            if (out.size() > bound) {
                printf("case %d frame %d: %zu bytes exceed the bound %llu\n", c, k, out.size(), (unsigned long long)bound);
                return 1;
            }
            printf("frame %d %d %zu ", c, k, out.size());
            for (uint8_t b : out) printf("%02x", b);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

// ---- PNG-8 image data ------------------------------------------------------------------------------------------
static int run_pngdeflate(const char *path, const int n_cases, const bool dynamic)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[5];   // frames, h, w, depth, seg_bytes
        if (fread(head, sizeof(int32_t), 5, f) != 5 || head[0] < 0 || !png_geometry_ok(head[1], head[2], head[3], head[4])) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const size_t n_px = (size_t)head[1] * (size_t)head[2];
        std::vector<uint8_t> plane(n_px), out;   // exactly n_px bytes: a read past the plane is a sanitizer report
        const uint64_t bound = png_deflate_bound(png_filtered_size(head[1], head[2], head[3]), head[4]);
        for (int k = 0; k < head[0]; ++k) {
            if (fread(plane.data(), 1, n_px, f) != n_px) {
                fprintf(stderr, "short record %d in %s\n", c, path);
                return 2;
            }
            png_deflate_encode_blocks(plane.data(), head[1], head[2], head[3], head[4], dynamic, out);
            if (out.size() > bound) {
                printf("case %d frame %d: %zu bytes exceed the bound %llu\n", c, k, out.size(), (unsigned long long)bound);
                return 1;
            }
            printf("frame %d %d %zu ", c, k, out.size());
            for (uint8_t b : out) printf("%02x", b);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

// ---- finished PNG chunks and their CRCs --------------------------------------------------------------------------
static int run_pngfile(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[8];   // frames, stride, n_idat, seq0, seq_step, pre_bytes, per-frame prefixes, post_bytes
        if (fread(head, sizeof(int32_t), 8, f) != 8 || head[0] < 0 || head[0] > 4096 || head[2] < 0 || head[2] > head[0] ||
            !png_file_geometry_ok(head[1], head[5], head[7])) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const size_t n = (size_t)head[0], stride = (size_t)head[1], pre_rows = head[6] ? n : 1;
        // exactly as many bytes as the statement may touch: anything past them is a sanitizer report
        std::vector<int64_t> sizes(n), offsets(n + 1, -1);
        std::vector<uint8_t> streams(n * stride), pre(pre_rows * (size_t)head[5]), post((size_t)head[7]);
        std::vector<uint8_t> out(n * (size_t)png_file_bound(head[1], head[5], head[7]));
        if (fread(sizes.data(), sizeof(int64_t), n, f) != n || fread(streams.data(), 1, streams.size(), f) != streams.size() ||
            fread(pre.data(), 1, pre.size(), f) != pre.size() || fread(post.data(), 1, post.size(), f) != post.size()) {
            fprintf(stderr, "short record %d in %s\n", c, path);
            return 2;
        }
        const int64_t total = png_file_assemble(streams.data(), head[1], sizes.data(), head[0], head[2], (uint32_t)head[3], (uint32_t)head[4], pre.data(),
                                                head[6] ? head[5] : 0, head[5], post.data(), head[7], out.data(), offsets.data());
        if (total < 0 || (size_t)total > out.size() || offsets[n] != total) {
            printf("case %d: %lld bytes against a bound of %zu\n", c, (long long)total, out.size());
            return 1;
        }
        printf("file %d %lld ", c, (long long)total);
        for (int64_t i = 0; i < total; ++i) printf("%02x", out[(size_t)i]);
        printf("\n");
        uint32_t joined = crc32_bytes(nullptr, 0);
        for (size_t r = 0; r < n; ++r) {
            const size_t len = (size_t)png_file_clamp(sizes[r], head[1]);
            const uint32_t one = crc32_bytes(streams.data() + r * stride, len);
            joined = crc32_combine(joined, one, len);
            printf("crc %d %zu %08x %08x\n", c, r, one, joined);   // the run's own, and that of all runs so far back to back
        }
    }
    fclose(f);
    return 0;
}

// ---- ordered dither: which kernel serves a call ------------------------------------------------------------------
static int run_orderedplan(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        OrderedFacts facts;
        OrderedSwitches sw;
        if (fread(&facts, sizeof(facts), 1, f) != 1 || fread(&sw, sizeof(sw), 1, f) != 1 || facts.hw < 1 || facts.w < 1 || facts.n_cus < 1) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const OrderedPlan p = plan_ordered(facts, sw);
        static const char *const tables[] = {"plain8", "plain4", "warped"};
        printf("plan %d %s %d %d %d %d %d %s %u %u %u %u %u %u %u %d %d %u\n", c, family_name(p.family), p.mode, p.bw, (int)p.adapt, (int)p.warp,
               (int)p.half, tables[p.table], p.grid, p.block, p.n_tiles, p.n_words, p.adv_y, p.adv_x, p.lds_bytes, p.fix_mode,
               (int)p.fix_big_queue, p.fix_grid);
    }
    fclose(f);
    return 0;
}

// ---- ordered dither: the fine table and the choice of its kernel ---------------------------------------------------
// N(x): the entries at the smallest distance; T(x): everything up to the second smallest (counted with multiplicity).  Only
// entries whose smallest distance to the cell is within the second smallest LARGEST distance of any entry can be members.
static void fine_masks(const std::vector<uint8_t> &pal, const int K, const int mw, std::vector<uint32_t> &tm, std::vector<uint32_t> &nm)
{
    tm.assign((size_t)kFineCells * mw, 0u);
    nm.assign((size_t)kFineCells * mw, 0u);
    parallel_cells(kFineCells, [&](const int lo, const int hi) {
        std::vector<int> cand, d;
        for (int cell = lo; cell < hi; ++cell) {
            const int c0[3] = {(cell & 31) * 8, ((cell >> 5) & 31) * 8, (cell >> 10) * 8};
            int u0 = 1 << 30, u1 = 1 << 30;  // the two smallest upper bounds
            std::vector<int> dmin(K);
            for (int j = 0; j < K; ++j) {
                int lo2 = 0, hi2 = 0;
                for (int k = 0; k < 3; ++k) {
                    const int p = pal[3 * j + k], a = c0[k], b = c0[k] + 7;
                    const int near = p < a ? a - p : (p > b ? p - b : 0), far = std::max(std::abs(p - a), std::abs(p - b));
                    lo2 += near * near;
                    hi2 += far * far;
                }
                dmin[j] = lo2;
                if (hi2 < u0) {
                    u1 = u0;
                    u0 = hi2;
                } else if (hi2 < u1) {
                    u1 = hi2;
                }
            }
            cand.clear();
            for (int j = 0; j < K; ++j)
                if (dmin[j] <= u1) cand.push_back(j);
            d.resize(cand.size());
            uint32_t *t = &tm[(size_t)cell * mw], *n = &nm[(size_t)cell * mw];
            for (int i = 0; i < 512; ++i) {
                const int r = c0[0] + (i & 7), g = c0[1] + ((i >> 3) & 7), b = c0[2] + (i >> 6);
                int d0 = 1 << 30, d1 = 1 << 30;
                for (size_t q = 0; q < cand.size(); ++q) {
                    const uint8_t *p = &pal[3 * (size_t)cand[q]];
                    d[q] = (r - p[0]) * (r - p[0]) + (g - p[1]) * (g - p[1]) + (b - p[2]) * (b - p[2]);
                    if (d[q] < d0) {
                        d1 = d0;
                        d0 = d[q];
                    } else if (d[q] < d1) {
                        d1 = d[q];
                    }
                }
                for (size_t q = 0; q < cand.size(); ++q) {
                    const int j = cand[q];
                    if (d[q] <= d1) t[j >> 5] |= 1u << (j & 31);
                    if (d[q] == d0) n[j >> 5] |= 1u << (j & 31);
                }
            }
        }
    });
}

static int run_finepack(const char *path, const int K, const char *out_path)
{
    if (K < 2 || K > 256) {
        fprintf(stderr, "finepack: 2 <= K <= 256\n");
        return 2;
    }
    std::vector<uint8_t> pal((size_t)K * 3);
    FILE *f = fopen(path, "rb");
    if (!f || fread(pal.data(), 1, pal.size(), f) != pal.size()) {
        fprintf(stderr, "cannot read %d colours from %s\n", K, path);
        return 2;
    }
    fclose(f);
    const int mw = 8;
    std::vector<uint32_t> coord4(K), tm, nm;
    for (int j = 0; j < K; ++j) coord4[j] = (uint32_t)pal[3 * j] | ((uint32_t)pal[3 * j + 1] << 8) | ((uint32_t)pal[3 * j + 2] << 16);
    fine_masks(pal, K, mw, tm, nm);
    FineTable ft, again;
    fine_pack(tm.data(), nm.data(), mw, K, coord4, fine_table_fits, ft);
    fine_pack(tm.data(), nm.data(), mw, K, coord4, fine_table_fits, again);  // the same answer every time
    const std::vector<uint32_t> im = ft.ok ? ft.lds_image() : std::vector<uint32_t>();
    int bad = ft.ok != again.ok || ft.off != again.off || ft.win_idx != again.win_idx || ft.wide_idx != again.wide_idx;
    if (ft.ok) bad += (int64_t)im.size() * 4 != fine_table_bytes(ft.n_win, ft.n_wide) || !fine_table_fits(ft.n_win, ft.n_wide);
    f = fopen(out_path, "wb");
    if (!f) return 2;
    const int32_t head[4] = {ft.ok ? 1 : 0, ft.n_win, ft.n_wide, (int32_t)im.size()};
    fwrite(head, sizeof(int32_t), 4, f);
    if (ft.ok) {
        fwrite(ft.off.data(), 2, ft.off.size(), f);
        fwrite(ft.win_idx.data(), 2, ft.win_idx.size(), f);
        fwrite(ft.wide_cell.data(), 2, ft.wide_cell.size(), f);
        fwrite(ft.wide_idx.data(), 2, ft.wide_idx.size(), f);
        fwrite(ft.quad.data(), 4, ft.quad.size(), f);
        fwrite(ft.pair.data(), 4, ft.pair.size(), f);
        fwrite(ft.wide.data(), 4, ft.wide.size(), f);
        fwrite(im.data(), 4, im.size(), f);
    }
    fclose(f);
    printf("finepack K=%d ok=%d windows=%d wide=%d bytes=%lld bad=%d\n", K, (int)ft.ok, ft.n_win, ft.n_wide,
           (long long)(ft.ok ? fine_table_bytes(ft.n_win, ft.n_wide) : 0), bad);
    return bad ? 1 : 0;
}

static int run_finesub(const char *path, const int K, const char *out_path)
{
    if (K < 2 || K > 256) {
        fprintf(stderr, "finesub: 2 <= K <= 256\n");
        return 2;
    }
    std::vector<uint8_t> pal((size_t)K * 3);
    FILE *f = fopen(path, "rb");
    if (!f || fread(pal.data(), 1, pal.size(), f) != pal.size()) {
        fprintf(stderr, "cannot read %d colours from %s\n", K, path);
        return 2;
    }
    fclose(f);
    const int mw = 8;
    std::vector<uint32_t> coord4(K), tm, nm;
    for (int j = 0; j < K; ++j) coord4[j] = (uint32_t)pal[3 * j] | ((uint32_t)pal[3 * j + 1] << 8) | ((uint32_t)pal[3 * j + 2] << 16);
    fine_masks(pal, K, mw, tm, nm);
    FineTable ft, again;
    fine_pack_sub(tm.data(), nm.data(), mw, K, coord4, fine_sub_fits, ft);
    fine_pack_sub(tm.data(), nm.data(), mw, K, coord4, fine_sub_fits, again);  // the same answer every time
    const std::vector<uint32_t> im = ft.ok ? ft.sub_image() : std::vector<uint32_t>();
    int bad = ft.ok != again.ok || ft.off != again.off || ft.rows != again.rows || ft.win_idx != again.win_idx || ft.wide_idx != again.wide_idx ||
              ft.sub_wide != again.sub_wide;
    if (ft.ok) {
        bad += (int64_t)im.size() * 4 != fine_sub_image_bytes(ft.n_win, ft.n_wide) || !fine_sub_fits(ft.n_win, ft.n_wide) || !ft.sub;
        // the sets of every sub-cell of a wide cell over the WHOLE palette: in its window (N in the quad), or the sub-cell is still wide
        size_t still = 0;
        for (int k = 0; k < ft.n_wide; ++k) {
            const int cell = ft.wide_cell[(size_t)k];
            bad += ft.off[(size_t)cell] != (uint16_t)(kFineSubTag | k);
            for (int sc = 0; sc < 8; ++sc) {
                std::vector<uint8_t> in_t((size_t)K, 0), in_n((size_t)K, 0);
                std::vector<int> d((size_t)K);
                for (int i = 0; i < 64; ++i) {
                    const int r = (cell & 31) * 8 + (sc & 1) * 4 + (i & 3), g = ((cell >> 5) & 31) * 8 + ((sc >> 1) & 1) * 4 + ((i >> 2) & 3),
                              b = (cell >> 10) * 8 + (sc >> 2) * 4 + (i >> 4);
                    bad += fine_cell(r, g, b) != cell || fine_sub_cell(r, g, b) != sc;
                    int d0 = 1 << 30, d1 = 1 << 30;
                    for (int j = 0; j < K; ++j) {
                        const uint8_t *q = &pal[3 * (size_t)j];
                        d[(size_t)j] = (r - q[0]) * (r - q[0]) + (g - q[1]) * (g - q[1]) + (b - q[2]) * (b - q[2]);
                        if (d[(size_t)j] < d0) d1 = d0, d0 = d[(size_t)j];
                        else if (d[(size_t)j] < d1) d1 = d[(size_t)j];
                    }
                    for (int j = 0; j < K; ++j) {
                        if (d[(size_t)j] <= d1) in_t[(size_t)j] = 1;
                        if (d[(size_t)j] == d0) in_n[(size_t)j] = 1;
                    }
                }
                int nt = 0, nn = 0;
                for (int j = 0; j < K; ++j) nt += in_t[(size_t)j], nn += in_n[(size_t)j];
                const uint16_t wi = ft.rows[(size_t)k * 8 + sc];
                const bool wide = nn > kFineQuad || nt > kFineWindow;
                if (wide) {
                    bad += wi != 0 || still >= ft.sub_wide.size() || ft.sub_wide[still] != (uint16_t)(8 * k + sc);
                    ++still;
                    continue;
                }
                bad += wi == 0 || wi >= ft.n_win;
                if (wi == 0 || wi >= ft.n_win) continue;
                const uint16_t *e = &ft.win_idx[(size_t)wi * kFineWindow];
                for (int j = 0; j < K; ++j) {
                    bool in_quad = false, in_win = false;
                    for (int q = 0; q < kFineWindow; ++q)
                        if (e[q] == j) in_win = true, in_quad = in_quad || q < kFineQuad;
                    bad += (in_n[(size_t)j] && !in_quad) || (in_t[(size_t)j] && !in_win);
                }
            }
        }
        bad += still != ft.sub_wide.size();
    }
    f = fopen(out_path, "wb");
    if (!f) return 2;
    const int32_t head[5] = {ft.ok ? 1 : 0, ft.n_win, ft.n_wide, (int32_t)ft.sub_wide.size(), (int32_t)im.size()};
    fwrite(head, sizeof(int32_t), 5, f);
    if (ft.ok) {
        fwrite(ft.off.data(), 2, ft.off.size(), f);
        fwrite(ft.rows.data(), 2, ft.rows.size(), f);
        fwrite(ft.win_idx.data(), 2, ft.win_idx.size(), f);
        fwrite(ft.wide_cell.data(), 2, ft.wide_cell.size(), f);
        fwrite(ft.sub_wide.data(), 2, ft.sub_wide.size(), f);
        fwrite(ft.wide_idx.data(), 2, ft.wide_idx.size(), f);
        fwrite(ft.quad.data(), 4, ft.quad.size(), f);
        fwrite(ft.pair.data(), 4, ft.pair.size(), f);
        fwrite(ft.wide.data(), 4, ft.wide.size(), f);
        fwrite(im.data(), 4, im.size(), f);
    }
    fclose(f);
    printf("finesub K=%d ok=%d windows=%d wide=%d still_wide=%zu bytes=%lld bad=%d\n", K, (int)ft.ok, ft.n_win, ft.n_wide, ft.sub_wide.size(),
           (long long)(ft.ok ? fine_sub_bytes(ft.n_win, ft.n_wide) : 0), bad);
    return bad ? 1 : 0;
}

static int run_fineaddr(const long first, const long n)
{
    if (first < 0 || n < 0 || first + n > (1L << 24)) {
        fprintf(stderr, "fineaddr: colours within 0 .. 2^24\n");
        return 2;
    }
    long bad_cell = 0, bad_row = 0, bad_tag = 0, rows = 0;
    for (long i = first; i < first + n; ++i) {
        const uint32_t x = (uint32_t)i;
        const uint32_t want = 2u * (uint32_t)fine_cell((int)(x & 255u), (int)((x >> 8) & 255u), (int)(x >> 16));
        bad_cell += fine_cell_offset(x) != want || fine_cell_offset(x, 73728u) != want + 73728u || fine_cell_offset(x | 0xa5000000u) != want;
    }
    const uint32_t rows_at[3] = {kFineRowsAt, 0x8000u, 147456u};  // where SUB 2 has the rows, the lowest address the form allows, a high one
    for (uint32_t rank = 0; rank < (uint32_t)kFineIds; ++rank) {
        const uint32_t tag = (uint32_t)kFineSubTag | rank, staged = fine_stage_tag(tag);
        bad_tag += staged > 0xffffu || staged <= (uint32_t)kFineSubTag - 1u || fine_tag_rank(staged) != rank;
        // two at a time, next to an ordinary window number on either side
        const uint32_t plain = 1u + (rank * 37u) % 0x7fffu;
        bad_tag += fine_stage_tags2(tag | (plain << 16)) != (staged | (plain << 16)) || fine_stage_tags2(plain | (tag << 16)) != (plain | (staged << 16)) ||
                   fine_stage_tags2(tag | (tag << 16)) != (staged | (staged << 16)) || fine_stage_tags2(plain | (plain << 16)) != (plain | (plain << 16));
        for (int sc = 0; sc < 8; ++sc)
            for (int j = 0; j < 64; ++j) {
                // the 64 colours of sub-cell sc of some cell (the cell does not enter the address)
                const int cell = (int)((rank * 61u + (uint32_t)sc * 4099u) % (uint32_t)kFineCells);
                const int r = (cell & 31) * 8 + (sc & 1) * 4 + (j & 3), g = ((cell >> 5) & 31) * 8 + ((sc >> 1) & 1) * 4 + ((j >> 2) & 3),
                          b = (cell >> 10) * 8 + (sc >> 2) * 4 + (j >> 4);
                const uint32_t x = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
                bad_row += fine_sub_cell(r, g, b) != sc;
                for (const uint32_t at : rows_at) bad_row += fine_row_address(staged, x, at) != at + 16u * rank + 2u * (uint32_t)sc;
                bad_row += (kFineRowsAt - (uint32_t)kFineSubTag) + fine_row_offset(staged, x | 0x5a000000u) != kFineRowsAt + 16u * rank + 2u * (uint32_t)sc;
                ++rows;
            }
    }
    printf("fineaddr colours=%ld rows=%ld bad_cell=%ld bad_row=%ld bad_tag=%ld\n", n, rows, bad_cell, bad_row, bad_tag);
    return bad_cell || bad_row || bad_tag ? 1 : 0;
}

static int run_finesublevel(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        FineSubFacts ff;
        if (fread(&ff, sizeof(ff), 1, f) != 1 || ff.n_win < 0 || ff.n_wide < 0 || ff.thr_bytes < 0) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            fclose(f);
            return 2;
        }
        printf("sub %d %d\n", c, fine_sub_level(ff));
    }
    fclose(f);
    return 0;
}

static int run_fineplan(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        OrderedFacts facts;
        OrderedSwitches sw;
        FineFacts ff;
        if (fread(&facts, sizeof(facts), 1, f) != 1 || fread(&sw, sizeof(sw), 1, f) != 1 || fread(&ff, sizeof(ff), 1, f) != 1 || facts.hw < 1 ||
            facts.w < 1 || facts.n_cus < 1) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const OrderedPlan p = plan_ordered(facts, sw);
        printf("fine %d %s %d\n", c, family_name(p.family), (int)fine_replaces(p, ff));
    }
    fclose(f);
    return 0;
}

static int run_finechoice(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        OrderedFacts facts;
        OrderedSwitches sw;
        FineTables ft;
        FineSwitches fsw;
        if (fread(&facts, sizeof(facts), 1, f) != 1 || fread(&sw, sizeof(sw), 1, f) != 1 || fread(&ft, sizeof(ft), 1, f) != 1 ||
            fread(&fsw, sizeof(fsw), 1, f) != 1 || facts.hw < 1 || facts.w < 1 || facts.n_cus < 1 || ft.n_win < 0 || ft.n_wide < 0 ||
            ft.sub_win < 0 || ft.sub_wide < 0 || ft.thr_bytes < 0) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            fclose(f);
            return 2;
        }
        const OrderedPlan p = plan_ordered(facts, sw);
        const FineChoice fc = choose_fine(p, ft, fsw);
        printf("choice %d %s %d %d %d %d %d\n", c, family_name(p.family), fc.fine, fc.keys, fc.sub, (int)fine_instance(fc.keys, fc.sub, false),
               (int)fine_instance(fc.keys, fc.sub, true));
    }
    fclose(f);
    return 0;
}

static int run_fixneeded(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        FixFacts ff;
        FixSwitches sw;
        if (fread(&ff, sizeof(ff), 1, f) != 1 || fread(&sw, sizeof(sw), 1, f) != 1 || ff.family < kFamBrute || ff.family > kFamCompactFloat ||
            ff.table < kTabPlain8 || ff.table > kTabWarped || ff.slow_blocks < 0) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            fclose(f);
            return 2;
        }
        printf("fix %d %s %d\n", c, family_name((OrderedFamily)ff.family), (int)fix_needed(ff, sw));
    }
    fclose(f);
    return 0;
}

static int run_finekeys(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        FineFacts ff;
        if (fread(&ff, sizeof(ff), 1, f) != 1 || ff.n_win < 0 || ff.thr_bytes < 0) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            fclose(f);
            return 2;
        }
        printf("keys %d %d\n", c, fine_keys_level(ff));
    }
    fclose(f);
    return 0;
}

// ---- void-and-cluster rank matrices ------------------------------------------------------------------------------
static int run_voidcluster(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[4];   // h, w, seed (its bits), sigma256
        if (fread(head, sizeof(int32_t), 4, f) != 4 || !vac_args_ok(head[0], head[1], head[3])) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const int n = head[0] * head[1];
        std::vector<uint16_t> ranks((size_t)n);   // exactly as many as the statement may write
        std::vector<float> thr((size_t)n);
        int rounds = 0;
        vac_generate(head[0], head[1], (uint32_t)head[2], head[3], ranks.data(), &rounds);
        vac_thresholds(ranks.data(), n, thr.data());
        printf("ranks %d %d", c, rounds);
        for (int i = 0; i < n; ++i) printf(" %u", (unsigned)ranks[(size_t)i]);
        printf("\nthr %d", c);
        for (int i = 0; i < n; ++i) {
            uint32_t bits;
            std::memcpy(&bits, &thr[(size_t)i], sizeof(bits));
            printf(" %08x", bits);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}

// ---- the Oklab colour metric ---------------------------------------------------------------------------------------
// record: K, n (int32), K * 3 float32 palette values, n float32 thresholds, n * 3 bytes of colours
static int run_metric(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[2];
        if (fread(head, sizeof(int32_t), 2, f) != 2 || head[0] < 1 || head[0] > 256 || head[1] < 0 || head[1] > (1 << 20)) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const int K = head[0], n = head[1];
        std::vector<float> pal((size_t)3 * K), thr((size_t)n);
        std::vector<uint8_t> rgb((size_t)3 * n);
        if (fread(pal.data(), sizeof(float), pal.size(), f) != pal.size() || fread(thr.data(), sizeof(float), thr.size(), f) != thr.size() ||
            fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || !metric_palette_ok(pal.data(), K)) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        std::vector<int32_t> lab((size_t)3 * n), coords((size_t)3 * K), d0((size_t)n), d1((size_t)n);   // exactly what the statements write
        std::vector<uint8_t> i0((size_t)n), i1((size_t)n);
        for (int i = 0; i < n; ++i) metric_lab(rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2], i & 1 ? metric_cbrt_table() : nullptr, &lab[3 * (size_t)i]);
        metric_palette_coords(pal.data(), K, 1, coords.data());
        metric_top2(rgb.data(), n, coords.data(), K, 1, i0.data(), i1.data(), d0.data(), d1.data());
        printf("lab %d", c);
        for (int i = 0; i < 3 * n; ++i) printf(" %d", lab[(size_t)i]);
        printf("\ntop %d", c);
        for (int i = 0; i < n; ++i) printf(" %u %u %d", (unsigned)i0[(size_t)i], (unsigned)i1[(size_t)i], (int)metric_takes_nearest(d0[(size_t)i], d1[(size_t)i], thr[(size_t)i]));
        printf("\n");
    }
    fclose(f);
    return 0;
}

// ---- integer error diffusion: the tap plan ---------------------------------------------------------------------------
// record: n_taps, divisor, strength256 (int32), then n_taps dx, n_taps dy, n_taps weights (int32)
static int run_idiffplan(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[3];
        if (fread(head, sizeof(int32_t), 3, f) != 3 || head[0] > 64) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const size_t n = head[0] > 0 ? (size_t)head[0] : 0;
        std::vector<int32_t> dx(n), dy(n), wt(n);   // exactly as many as the plan may read
        if (fread(dx.data(), sizeof(int32_t), n, f) != n || fread(dy.data(), sizeof(int32_t), n, f) != n || fread(wt.data(), sizeof(int32_t), n, f) != n) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        IdiffPlan p;
        const int rc = idiff_plan(dx.data(), dy.data(), wt.data(), head[0], head[1], head[2], p);
        printf("idiff %d %d %d %d", c, rc, p.n, p.skew);
        for (int k = 0; k < p.n; ++k) printf(" %u", (unsigned)p.q[k]);
        printf("\n");
    }
    fclose(f);
    return 0;
}

// ---- Oklab palette fitting: the host statement -------------------------------------------------------------------------
// record: n, K, max_iter (int32), then n codes, n counts (uint32)
static int run_okfit(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[3];
        if (fread(head, sizeof(int32_t), 3, f) != 3 || head[0] < 0 || head[0] > (1 << 24)) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const size_t n = (size_t)head[0];
        std::vector<uint32_t> codes(n), counts(n);   // exactly as many as the statement may read
        if (fread(codes.data(), sizeof(uint32_t), n, f) != n || fread(counts.data(), sizeof(uint32_t), n, f) != n) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const int K = head[1], rule = okfit_check(codes.data(), counts.data(), (int64_t)n, K, head[2]);
        printf("okfit %d %d", c, rule);
        if (!rule) {
            std::vector<uint8_t> pal((size_t)3 * K);   // exactly what the statement writes
            std::vector<int32_t> centres((size_t)3 * K);
            int n_iter = 0;
            uint64_t distortion = 0;
            okfit_host(codes.data(), counts.data(), (int64_t)n, K, head[2], pal.data(), centres.data(), &n_iter, &distortion);
            printf(" %d %llu", n_iter, (unsigned long long)distortion);
            for (int i = 0; i < 3 * K; ++i) printf(" %u", (unsigned)pal[(size_t)i]);
            for (int i = 0; i < 3 * K; ++i) printf(" %d", centres[(size_t)i]);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}

// ---- filtered resize: the coefficient tables, the plan and the host statement ------------------------------------------------
// resamplecoeffs record: in, out, filter (int32)
static int run_resamplecoeffs(const char *path, const int n_cases)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[3];
        if (fread(head, sizeof(int32_t), 3, f) != 3 || head[0] < 1 || head[1] < 1 || head[0] > kResampleMaxSize || head[1] > kResampleMaxSize ||
            head[2] < 0 || head[2] >= kResampleFilters) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        std::vector<int32_t> bounds, kk;
        const int ksize = resample_coeffs(head[0], head[1], head[2], bounds, kk);
        printf("coeffs %d %d", c, ksize);
        for (const int32_t v : bounds) printf(" %d", v);
        for (const int32_t v : kk) printf(" %d", v);
        printf("\n");
    }
    fclose(f);
    return 0;
}

// resample record: filter, n, h, w, oh, ow (int32), then n * h * w * 3 bytes; the output bytes of the accepted cases go to out_path
// back to back
static int run_resample(const char *path, const int n_cases, const char *out_path)
{
    FILE *f = fopen(path, "rb");
    FILE *g = fopen(out_path, "wb");
    if (!f || !g) {
        fprintf(stderr, "cannot open %s or %s\n", path, out_path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[6];
        if (fread(head, sizeof(int32_t), 6, f) != 6 || head[1] < 0 || head[1] > 64) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        ResamplePlanHost p;
        const int rule = resample_plan(head[0], head[2], head[3], head[4], head[5], p);
        printf("resample %d %d", c, rule);
        if (!rule) {
            const size_t nin = (size_t)head[1] * 3u * (size_t)p.h * (size_t)p.w, nout = (size_t)head[1] * 3u * (size_t)p.oh * (size_t)p.ow;
            std::vector<uint8_t> in(nin), out(nout);   // exactly what the statement reads and writes
            if (fread(in.data(), 1, nin, f) != nin) {
                fprintf(stderr, "bad record %d in %s\n", c, path);
                return 2;
            }
            resample_host(p, in.data(), out.data(), head[1]);
            if (fwrite(out.data(), 1, nout, g) != nout) return 2;
            printf(" %d %d %d %d %d %d %lld %lld", p.y0, p.y1, p.need_h ? 1 : 0, p.need_v ? 1 : 0, p.mul32 ? 1 : 0, p.h_kernel,
                   (long long)std::max(p.ver.max_abs, p.hor.max_abs), (long long)std::max(p.need_v ? p.ver.max_sum : 0, p.hor.max_sum));
        }
        printf("\n");
    }
    fclose(f);
    fclose(g);
    return 0;
}

// ---- temporal hold: the host statement -------------------------------------------------------------------------------------------
// hold record: n, h, w, cell, tol, share256, has_state, cut (int32), then n*h*w*3 source bytes, n*h*w plane bytes, h*w*3 anchor bytes
// and h*w held bytes (the state is read from the record whatever has_state says: without state it must not matter).  The batch goes
// through hold_apply as one call (cut < 0) or as the frames [0, cut) and [cut, n).  Per accepted case out_path gets n*h*w out
// bytes, n int64 counts, the anchor and the held plane, back to back; every vector has exactly the stated size.
static int run_hold(const char *path, const int n_cases, const char *out_path)
{
    FILE *f = fopen(path, "rb");
    FILE *g = fopen(out_path, "wb");
    if (!f || !g) {
        fprintf(stderr, "cannot open %s or %s\n", path, out_path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[8];
        if (fread(head, sizeof(int32_t), 8, f) != 8) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const int n = head[0], h = head[1], w = head[2], cell = head[3], tol = head[4], share256 = head[5], cut = head[7];
        const int rule = hold_rule(n, h, w, cell, tol, share256);
        printf("hold %d %d", c, rule);
        if (!rule) {
            if (n > 64 || cut > n) {
                fprintf(stderr, "bad record %d in %s\n", c, path);
                return 2;
            }
            const size_t px = (size_t)h * (size_t)w;
            std::vector<uint8_t> src((size_t)n * px * 3u), planes((size_t)n * px), anchor(px * 3u), held(px), out((size_t)n * px);
            std::vector<int64_t> refreshed((size_t)n, -1);
            if (fread(src.data(), 1, src.size(), f) != src.size() || fread(planes.data(), 1, planes.size(), f) != planes.size() ||
                fread(anchor.data(), 1, anchor.size(), f) != anchor.size() || fread(held.data(), 1, held.size(), f) != held.size()) {
                fprintf(stderr, "bad record %d in %s\n", c, path);
                return 2;
            }
            bool state = head[6] != 0;
            const int k = cut < 0 ? n : cut;
            if (k > 0) {   // exactly the frames of the call: a vector per call, so that a read past them is seen
                const std::vector<uint8_t> s(src.begin(), src.begin() + (ptrdiff_t)((size_t)k * px * 3u)), p(planes.begin(), planes.begin() + (ptrdiff_t)((size_t)k * px));
                std::vector<uint8_t> o((size_t)k * px);
                hold_apply(s.data(), p.data(), k, h, w, cell, tol, share256, anchor.data(), held.data(), state, o.data(), refreshed.data());
                std::copy(o.begin(), o.end(), out.begin());
                state = true;
            }
            if (n - k > 0) {
                const std::vector<uint8_t> s(src.begin() + (ptrdiff_t)((size_t)k * px * 3u), src.end()), p(planes.begin() + (ptrdiff_t)((size_t)k * px), planes.end());
                std::vector<uint8_t> o((size_t)(n - k) * px);
                std::vector<int64_t> r((size_t)(n - k), -1);
                hold_apply(s.data(), p.data(), n - k, h, w, cell, tol, share256, anchor.data(), held.data(), state, o.data(), r.data());
                std::copy(o.begin(), o.end(), out.begin() + (ptrdiff_t)((size_t)k * px));
                std::copy(r.begin(), r.end(), refreshed.begin() + k);
            }
            if (fwrite(out.data(), 1, out.size(), g) != out.size() || fwrite(refreshed.data(), sizeof(int64_t), refreshed.size(), g) != refreshed.size() ||
                fwrite(anchor.data(), 1, anchor.size(), g) != anchor.size() || fwrite(held.data(), 1, held.size(), g) != held.size())
                return 2;
            long long total = 0;
            for (const int64_t v : refreshed) total += v;
            printf(" %lld", total);
        }
        printf("\n");
    }
    fclose(f);
    fclose(g);
    return 0;
}

// ---- transparency: the host statements ---------------------------------------------------------------------------------------------
// alpha record: n, h, w, mode, threshold, m, y0, x0, has_matte, key (int32), 3 matte bytes, 3 fill bytes, then (accepted cases only)
// n*h*w*4 RGBA bytes.  The frames go through alpha_split; the planes of the key are the red channel mod 200, keyed with the mask the
// split made; the join takes the split's RGB and mask.  Per accepted case out_path gets the RGB, the mask, n int64 counts, the keyed
// planes and the RGBA, back to back; every vector has exactly the stated size.
static int run_alpha(const char *path, const int n_cases, const char *out_path)
{
    FILE *f = fopen(path, "rb");
    FILE *g = fopen(out_path, "wb");
    if (!f || !g) {
        fprintf(stderr, "cannot open %s or %s\n", path, out_path);
        return 2;
    }
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[10];
        uint8_t colours[6];
        if (fread(head, sizeof(int32_t), 10, f) != 10 || fread(colours, 1, 6, f) != 6) {
            fprintf(stderr, "bad record %d in %s\n", c, path);
            return 2;
        }
        const int n = head[0], h = head[1], w = head[2], mode = head[3], threshold = head[4], m = head[5], y0 = head[6], x0 = head[7], key = head[9];
        int rule = alpha_geometry_rule(n, h, w);
        if (!rule) rule = alpha_split_rule(mode, threshold, m, y0, x0);
        printf("alpha %d %d", c, rule);
        if (!rule) {
            if (n > 64 || key < 0 || key > 255) {
                fprintf(stderr, "bad record %d in %s\n", c, path);
                return 2;
            }
            const size_t px = (size_t)n * (size_t)h * (size_t)w;
            std::vector<uint8_t> rgba(px * 4u), rgb(px * 3u), mask(px), planes(px), keyed(px), joined(px * 4u);
            std::vector<int64_t> masked((size_t)n, -1);
            if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size()) {
                fprintf(stderr, "bad record %d in %s\n", c, path);
                return 2;
            }
            alpha_split(rgba.data(), n, h, w, mode, threshold, m, mode == 1 ? y0 : 0, mode == 1 ? x0 : 0, head[8] != 0, colours, rgb.data(), mask.data(),
                        masked.data());
            for (size_t i = 0; i < px; ++i) planes[i] = (uint8_t)(rgba[4 * i] % 200);
            alpha_key(planes.data(), mask.data(), px, key, keyed.data());
            alpha_join(rgb.data(), mask.data(), px, colours + 3, joined.data());
            if (fwrite(rgb.data(), 1, rgb.size(), g) != rgb.size() || fwrite(mask.data(), 1, mask.size(), g) != mask.size() ||
                fwrite(masked.data(), sizeof(int64_t), masked.size(), g) != masked.size() || fwrite(keyed.data(), 1, keyed.size(), g) != keyed.size() ||
                fwrite(joined.data(), 1, joined.size(), g) != joined.size())
                return 2;
            long long total = 0;
            for (const int64_t v : masked) total += v;
            printf(" %lld", total);
        }
        printf("\n");
    }
    fclose(f);
    fclose(g);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s kdtree|edtables|accel <pts.f64> <K> [bw]  |  edtablesdigest <pts.f64> <K> <what>  |  mediancut <rgb.u8> <n> <depth>  |  indexmap <lists.bin> <n>  |  giflzw <cases.bin> <n>  |  pngdeflate|pngdyn|pngfile <cases.bin> <n>  |  orderedplan <cases.bin> <n>  |  voidcluster <cases.bin> <n>  |  metric <cases.bin> <n>  |  finepack <pal.u8> <K> <out.bin>  |  fineplan <cases.bin> <n>  |  finekeys <cases.bin> <n>  |  finesub <pal.u8> <K> <out.bin>  |  finesublevel <cases.bin> <n>  |  finechoice <cases.bin> <n>  |  fineaddr <first> <n>  |  fixneeded <cases.bin> <n>  |  idiffplan <cases.bin> <n>  |  okfit <cases.bin> <n>  |  resamplecoeffs <cases.bin> <n>  |  resample <cases.bin> <n> <out.bin>  |  hold <cases.bin> <n> <out.bin>  |  alpha <cases.bin> <n> <out.bin>\n", argv[0]);
        return 2;
    }
    if (std::string(argv[1]) == "mediancut") return run_mediancut(argv[2], atol(argv[3]), argc > 4 ? atoi(argv[4]) : 4);
    if (std::string(argv[1]) == "indexmap") return run_indexmap(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "giflzw") return run_giflzw(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "pngdeflate") return run_pngdeflate(argv[2], atoi(argv[3]), false);
    if (std::string(argv[1]) == "pngdyn") return run_pngdeflate(argv[2], atoi(argv[3]), true);
    if (std::string(argv[1]) == "pngfile") return run_pngfile(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "orderedplan") return run_orderedplan(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "voidcluster") return run_voidcluster(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "metric") return run_metric(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "finepack") return argc > 4 ? run_finepack(argv[2], atoi(argv[3]), argv[4]) : 2;
    if (std::string(argv[1]) == "fineplan") return run_fineplan(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "finekeys") return run_finekeys(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "finesub") return argc > 4 ? run_finesub(argv[2], atoi(argv[3]), argv[4]) : 2;
    if (std::string(argv[1]) == "finesublevel") return run_finesublevel(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "finechoice") return run_finechoice(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "fineaddr") return run_fineaddr(atol(argv[2]), atol(argv[3]));
    if (std::string(argv[1]) == "fixneeded") return run_fixneeded(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "idiffplan") return run_idiffplan(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "okfit") return run_okfit(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "resamplecoeffs") return run_resamplecoeffs(argv[2], atoi(argv[3]));
    if (std::string(argv[1]) == "resample") return argc > 4 ? run_resample(argv[2], atoi(argv[3]), argv[4]) : 2;
    if (std::string(argv[1]) == "hold") return argc > 4 ? run_hold(argv[2], atoi(argv[3]), argv[4]) : 2;
    if (std::string(argv[1]) == "alpha") return argc > 4 ? run_alpha(argv[2], atoi(argv[3]), argv[4]) : 2;
    const int K = atoi(argv[3]);
    if (K < 1 || K > 1024) return 2;
    const std::vector<double> pts = read_pts(argv[2], K);
    const std::string cmd = argv[1];
    if (cmd == "kdtree") return run_kdtree(pts, K);
    if (cmd == "edtables") return run_edtables(pts, K);
    if (cmd == "edtablesdigest") return run_edtablesdigest(pts, K, argc > 4 ? atoi(argv[4]) : 3);
    if (cmd == "accel") return run_accel(pts, K, argc > 4 ? atoi(argv[4]) : 8);
    return 2;
}
