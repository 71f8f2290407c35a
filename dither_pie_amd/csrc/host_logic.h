// Host-side logic of libditherpie_hip.so that never touches the GPU: the scipy-order KD-tree build, the assembly of
// the search accelerator's cell table from membership masks, and (ed_tables.h) the candidate tables of the diffusion kernels with
// their multi-threaded per-cell loops.  Pure C++17, no HIP headers: included by the .hip / .cpp translation units through
// dp_internal.h AND compiled on its own under AddressSanitizer + UBSan and under ThreadSanitizer
// (`make host_asan host_tsan` -> build/host_asan, build/host_tsan from host_sanitize.cpp; run by
// tests/test_host_sanitizers.py in the CPU tier).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <numeric>
#include <thread>
#include <utility>
#include <exception>
#include <vector>

#include "../../include/ditherpie_hip.h"
#include "ed_tables.h"   // the candidate tables of the diffusion kernels

namespace dp {

constexpr int kLeafSize = 10;     // scipy.spatial.KDTree default (dithering_lib.py:339)
constexpr int kWideList = 16;     // entries of the flat candidate list of a split cell (ordered_fast_kernel, accel.hip)
constexpr int kQueueSmall = 64;   // traversal queue entries: every balanced tree of K <= 256 has <= 51 inner nodes
constexpr int kQueueLarge = 256;  // ... larger palettes (K <= 1024) and degenerate trees use the large instantiation

// KD-tree as scipy builds it; node 0 is the root, children follow in pre-order.
struct HostTree {
    int K = 0;
    std::vector<double> pts;  // K*3
    std::vector<int32_t> indices;
    std::vector<int32_t> split_dim, start, end, less, greater;
    std::vector<double> split;
    double mins[3], maxes[3];
};


// ---------------------------------------------------------------------------------------------
// scipy.spatial.KDTree(points) with its defaults (leafsize=10, compact_nodes, balanced_tree), the
// structure behind every palette search of the reference (dithering_lib.py:339, 358, 554, 655).
// The permutation std::nth_element leaves behind decides scipy's tie order, so the same standard
// algorithm (libstdc++ introselect) is used here, with scipy's coordinate-only comparator.
// ---------------------------------------------------------------------------------------------
namespace kd_detail {
struct Builder {
    HostTree &t;
    const double *P;

    double coord(int i, int d) const { return P[(size_t)i * 3 + d]; }

    // two-pointer partition of indices[s,e) by coord < split; returns the first index of the >= part
    int split_range(int s, int e, int d, double split)
    {
        int lo = s, hi = e - 1;
        while (lo <= hi) {
            if (coord(t.indices[lo], d) < split)
                ++lo;
            else if (coord(t.indices[hi], d) >= split)
                --hi;
            else
                std::swap(t.indices[lo++], t.indices[hi--]);
        }
        return lo;
    }

    int add_node(int s, int e)
    {
        int id = (int)t.split_dim.size();
        t.split_dim.push_back(-1);
        t.split.push_back(0.0);
        t.start.push_back(s);
        t.end.push_back(e);
        t.less.push_back(-1);
        t.greater.push_back(-1);
        return id;
    }

    int build(int s, int e)
    {
        const int id = add_node(s, e);
        if (e - s <= kLeafSize) return id;

        double lo[3], hi[3];
        for (int d = 0; d < 3; ++d) lo[d] = hi[d] = coord(t.indices[s], d);
        for (int j = s + 1; j < e; ++j)
            for (int d = 0; d < 3; ++d) {
                const double v = coord(t.indices[j], d);
                hi[d] = hi[d] > v ? hi[d] : v;
                lo[d] = lo[d] < v ? lo[d] : v;
            }
        int dim = 0;
        double extent = 0;
        for (int d = 0; d < 3; ++d)
            if (hi[d] - lo[d] > extent) {
                dim = d;
                extent = hi[d] - lo[d];
            }
        if (hi[dim] == lo[dim]) return id;  // all points coincide

        int32_t *first = t.indices.data() + s;
        const int half = (e - s) / 2;
        std::nth_element(first, first + half, first + (e - s),
                         [&](int32_t a, int32_t b) { return coord(a, dim) < coord(b, dim); });
        double split = coord(t.indices[s + half], dim);
        int cut = split_range(s, e, dim, split);
        if (cut == s) {
            // nothing lies strictly below the median value: cut just above the minimum instead
            double mn = coord(t.indices[s], dim);
            for (int j = s + 1; j < e; ++j) mn = std::min(mn, coord(t.indices[j], dim));
            split = std::nextafter(mn, std::numeric_limits<double>::infinity());
            cut = split_range(s, e, dim, split);
        }
        t.split_dim[id] = dim;
        t.split[id] = split;
        const int l = build(s, cut);
        const int g = build(cut, e);
        t.less[id] = l;
        t.greater[id] = g;
        return id;
    }
};
}  // namespace kd_detail

inline void build_tree(const double *pts, int K, HostTree &t)
{
    t = HostTree();
    t.K = K;
    t.pts.assign(pts, pts + (size_t)K * 3);
    t.indices.resize(K);
    std::iota(t.indices.begin(), t.indices.end(), 0);
    for (int d = 0; d < 3; ++d) t.mins[d] = t.maxes[d] = pts[d];
    for (int j = 1; j < K; ++j)
        for (int d = 0; d < 3; ++d) {
            t.mins[d] = std::min(t.mins[d], pts[(size_t)j * 3 + d]);
            t.maxes[d] = std::max(t.maxes[d], pts[(size_t)j * 3 + d]);
        }
    kd_detail::Builder b{t, t.pts.data()};
    b.build(0, K);
}


// Position of a 16x16x16 cell in the LDS table: the kernels form it as r' | b'<<4 | g'<<8 (x & 0xf0f0f0,
// OR-ed with itself shifted left by 12, bits 16..27), three operations fewer than r'<<8 | g'<<4 | b'.
inline int cell_slot(int rc, int gc, int bc) { return rc | (bc << 4) | (gc << 8); }


// an axis-aligned box of colours (the accelerator's octree below the 16^3 cells)
struct Box {
    int r0, g0, b0, size;
};


constexpr int kCells = 4096;
constexpr int kWideCap = 512;   // such lists per table at most
constexpr int kNearSlots = 6;  // entries of an 8-entry block that the nearest-only path of ordered_fast_kernel reads
constexpr int kTabCapWords = (160 * 1024 - 2048) / 4;  // LDS budget of the dither kernels
constexpr int kTabMaxWords = 1 << 20;                 // largest table built (4 MB); what exceeds LDS stays in global memory
// words the lean kernels stage when the table is larger than LDS: the 4096 cell blocks + the first split nodes
constexpr int kTabStageWords = 4096 * 8 + 88 * 64;

struct TableStats {
    int n_split = 0, n_slow = 0, max_cnt = 0, max_near = 0, n_near_overflow = 0;
    bool wide_overflow = false;
    std::vector<Box> node_box;  // the box each split node covers, by node index
    int n_split_cells = 0;  // 16^3 cells that are split (the pixels of these cells leave the main path of the kernels)
    bool too_big = false;
};

// Turns the per-cell membership masks into the LDS table: [4096 cells][8 words], then [n_split][8 sub-cells][8].
// coord4[j]: integer coordinates r | g<<8 | b<<16 of entry j (used to choose padding entries); word[j]: what a
// block stores for entry j.  box_masks(boxes, out) computes the membership masks (8 words each) of further boxes.
// nmasks (optional): the nearest sets N(cell) of the 4096 cells.  With them a cell whose N has more than `ns` members is
// split like an overflowing one, and perm[slot] receives, for every unsplit cell block, the order in which the fast
// ordered kernel stages the block's entries into LDS -- the members of N first (field k, 3 bits for bw = 8, 2 bits
// for bw = 4: which entry of the index-ordered block goes to LDS slot k; bits 28..31: |N|); 0xffffffff = split cell.
// The table itself stays in palette-index order (the tie codes are defined on that order).
// wide (with perm): for every SPLIT cell the whole list T(cell) in index order, padded to kWideList entries -- the fast
// kernel resolves the pixels of split cells on it (one block read instead of a descent through the octree);
// perm[slot] = 0xff000000 | list number.  A cell with a longer list sets st.wide_overflow (no fast kernel then).
template <class BoxMasks>
int assemble_table(const std::vector<uint32_t> &masks, const int mw, const int bw, const int cap_words, const int K,
                   const std::vector<uint32_t> &coord4, const std::vector<uint32_t> &word, BoxMasks box_masks,
                   std::vector<uint32_t> &tab, TableStats &st, const uint32_t *nmasks = nullptr, const int ns = 0,
                   std::vector<uint32_t> *perm = nullptr, std::vector<uint32_t> *wide = nullptr)
{
    // bw: entries per block (8, or 4 for small palettes); a split node is 8 child blocks
    tab.assign((size_t)kCells * bw, 0u);
    std::vector<int> list, extra;
    std::vector<uint64_t> dkey;
    // members of a mask, padded to bw with unused entries; false if more than bw
    auto make_block = [&](const uint32_t *mask, int cr, int cg, int cb, uint32_t *out8) {
        list.clear();
        for (int wi = 0; wi < mw && 32 * wi < K; ++wi)   // the members: the set bits of the mask below K
            for (uint32_t bits = mask[wi]; bits; bits &= bits - 1u) {
                const int j = 32 * wi + __builtin_ctz(bits);
                if (j < K) list.push_back(j);
            }
        st.max_cnt = std::max(st.max_cnt, (int)list.size());
        if (list.size() > (size_t)bw) return false;
        if (list.size() < (size_t)bw) {
            extra.clear();   // the lowest unused indices, as many as the padding needs
            for (int j = 0; j < K && extra.size() < (size_t)bw; ++j)
                if (!(mask[j >> 5] >> (j & 31) & 1u)) extra.push_back(j);
            // pad with unused entries: ANY real entry is harmless (it is not among the three nearest of any colour of the box, so its
            // key never decides anything), so the lowest unused indices do.  Rounds 2-5 took the unused entries nearest to the
            // centre -- a distance key for every unused entry of every cell and a partial sort: 3 of the 4.4 ms this assembly took
            // for 256 colours (tools/bench_scripts/accel_build_stages.py).
            const size_t need = (size_t)bw - list.size();
            (void)cr, (void)cg, (void)cb;
            for (size_t q = 0; q < need; ++q) list.push_back(extra[q]);
            std::sort(list.begin(), list.end());  // key ties must break towards the lower palette index
        }
        for (int i = 0; i < bw; ++i) out8[i] = word[list[i]];
        return true;
    };
    // pending splits below the 8^3 level: (block position in tab, box) resolved level by level
    struct Pending {
        size_t pos;
        Box box;
    };
    std::vector<Pending> pending;
    // turn the block at `pos` into a split node with 8 children of half size; children masks come
    // either from `child_masks` (8 x 8 words) or, if null, are requested for the next round
    auto split = [&](size_t pos, const Box &bx, const uint32_t *child_masks) {
        const size_t base = tab.size();
        if (base + 8 * (size_t)bw > (size_t)cap_words) {
            st.too_big = true;
            return;
        }
        tab.resize(base + 8 * (size_t)bw, 0u);
        tab[pos] = 0x80000000u | (uint32_t)((base - (size_t)kCells * bw) / (8 * (size_t)bw));
        ++st.n_split;
        st.node_box.push_back(bx);
        const int hs = bx.size / 2;
        for (int sidx = 0; sidx < 8; ++sidx) {
            Box c{bx.r0 + ((sidx >> 2) & 1) * hs, bx.g0 + ((sidx >> 1) & 1) * hs, bx.b0 + (sidx & 1) * hs, hs};
            const size_t cpos = base + (size_t)sidx * bw;
            if (child_masks) {
                uint32_t blk[8];
                if (make_block(child_masks + (size_t)mw * sidx, c.r0 + hs / 2, c.g0 + hs / 2, c.b0 + hs / 2, blk))
                    std::copy(blk, blk + bw, tab.begin() + cpos);
                else
                    pending.push_back({cpos, c});
            } else {
                pending.push_back({cpos, c});
            }
        }
    };
    if (perm) perm->assign(kCells, 0xffffffffu);
    for (int cell = 0; cell < kCells && !st.too_big; ++cell) {
        const uint32_t *m = &masks[(size_t)cell * 9 * mw];
        const int r0 = (cell >> 8) * 16, g0 = ((cell >> 4) & 15) * 16, b0 = (cell & 15) * 16;
        uint32_t blk[8];
        const size_t slot = (size_t)cell_slot(cell >> 8, (cell >> 4) & 15, cell & 15);
        bool fits = make_block(m, r0 + 8, g0 + 8, b0 + 8, blk);
        bool near_overflow = false;
        if (fits && nmasks) {
            // `list` holds the block's entries in index order: the nearest set first
            const uint32_t *nm = nmasks + (size_t)cell * mw;
            const int fb = bw == 8 ? 3 : 2;
            uint32_t pw = 0;
            int k = 0, n_near = 0;
            for (int pass = 0; pass < 2; ++pass)
                for (int i = 0; i < bw; ++i) {
                    const int j = list[i];
                    const bool near = (nm[j >> 5] >> (j & 31)) & 1u;
                    if (near == (pass == 0)) {
                        pw |= (uint32_t)i << (fb * k++);
                        n_near += near;
                    }
                }
            // a nearest set larger than the nearest-only path of the fast kernel reads: the cell keeps its block in the table,
            // but the fast kernel treats it as split (staging order = flat list below)
            near_overflow = n_near > ns;
            if (!near_overflow && perm) (*perm)[slot] = pw | ((uint32_t)n_near << 28);
            st.max_near = std::max(st.max_near, n_near);
            st.n_near_overflow += near_overflow;
        }
        if (fits) std::copy(blk, blk + bw, tab.begin() + slot * bw);
        if (!fits || near_overflow) {
            if (perm && wide) {
                // the cell's whole list, index order, padded with the unused entries nearest to the centre
                list.clear();
                extra.clear();
                for (int j = 0; j < K; ++j) ((m[j >> 5] >> (j & 31) & 1u) ? list : extra).push_back(j);
                if (K <= kWideList) {
                    // the whole palette (the kernel reads min(K, kWideList) entries)
                    (*perm)[slot] = 0xff000000u | (uint32_t)(wide->size() / kWideList);
                    for (int i = 0; i < kWideList; ++i) wide->push_back(i < K ? word[i] : 0u);
                } else if ((int)list.size() > kWideList) {
                    st.wide_overflow = true;
                } else {
                    const size_t need = (size_t)kWideList - list.size();
                    dkey.resize(extra.size());
                    for (size_t q = 0; q < extra.size(); ++q) {
                        const uint32_t c = coord4[extra[q]];
                        const int r = c & 255, g = (c >> 8) & 255, b = (c >> 16) & 255;
                        dkey[q] = ((uint64_t)((r - r0 - 8) * (r - r0 - 8) + (g - g0 - 8) * (g - g0 - 8) + (b - b0 - 8) * (b - b0 - 8)) << 16) | (uint64_t)extra[q];
                    }
                    std::partial_sort(dkey.begin(), dkey.begin() + need, dkey.end());
                    for (size_t q = 0; q < need; ++q) list.push_back((int)(dkey[q] & 0xffff));
                    std::sort(list.begin(), list.end());
                    (*perm)[slot] = 0xff000000u | (uint32_t)(wide->size() / kWideList);
                    for (int i = 0; i < kWideList; ++i) wide->push_back(word[list[i]]);
                }
            }
        }
        if (!fits) {
            split(slot * bw, Box{r0, g0, b0, 16}, m + mw);
            ++st.n_split_cells;
        }
    }
    // deeper levels: boxes that still hold more than 8 members are split again; a single colour that still
    // overflows is left to the fix-up pass
    while (!pending.empty() && !st.too_big) {
        std::vector<Pending> todo;
        todo.swap(pending);
        std::vector<Pending> kids;  // children whose masks we need this round
        for (const Pending &pd : todo) {
            if (pd.box.size == 1) {
                tab[pd.pos] = 0xC0000000u;
                ++st.n_slow;
                continue;
            }
            const size_t before = pending.size();
            split(pd.pos, pd.box, nullptr);
            if (st.too_big) break;
            for (size_t q = before; q < pending.size(); ++q) kids.push_back(pending[q]);
            pending.resize(before);
        }
        if (st.too_big || kids.empty()) break;
        std::vector<Box> boxes(kids.size());
        for (size_t q = 0; q < kids.size(); ++q) boxes[q] = kids[q].box;
        std::vector<uint32_t> bm(kids.size() * (size_t)mw);
        const int rc = box_masks(boxes, bm);
        if (rc != DP_OK) return rc;
        for (size_t q = 0; q < kids.size(); ++q) {
            const Box &c = kids[q].box;
            uint32_t blk[8];
            if (make_block(&bm[q * (size_t)mw], c.r0 + c.size / 2, c.g0 + c.size / 2, c.b0 + c.size / 2, blk))
                std::copy(blk, blk + bw, tab.begin() + kids[q].pos);
            else
                pending.push_back(kids[q]);
        }
    }
    return DP_OK;
}

// Tables larger than LDS: the kernels stage the cell blocks and the FIRST split nodes, the rest is read from global
// memory.  Put the nodes of the most crowded boxes first -- a palette extracted from an image crowds its colours where
// the image's pixels are, so those are the nodes the pixels visit.
inline void crowded_nodes_first(std::vector<uint32_t> &tab, const TableStats &st, const int bw, const std::vector<uint32_t> &coord4)
{
    const size_t n = st.node_box.size();
    if (n < 2) return;
    std::vector<int> score(n, 0);
    for (size_t k = 0; k < n; ++k) {
        const Box &b = st.node_box[k];
        for (const uint32_t c : coord4) {
            const int r = c & 255, g = (c >> 8) & 255, bl = (c >> 16) & 255;
            score[k] += (r >= b.r0 && r < b.r0 + b.size && g >= b.g0 && g < b.g0 + b.size && bl >= b.b0 && bl < b.b0 + b.size);
        }
    }
    std::vector<uint32_t> order(n), where(n);
    for (size_t k = 0; k < n; ++k) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });
    for (size_t k = 0; k < n; ++k) where[order[k]] = (uint32_t)k;
    const size_t base = (size_t)kCells * bw, node_words = 8 * (size_t)bw;
    std::vector<uint32_t> moved(tab.size());
    std::copy(tab.begin(), tab.begin() + base, moved.begin());
    for (size_t k = 0; k < n; ++k)
        std::copy(tab.begin() + base + k * node_words, tab.begin() + base + (k + 1) * node_words,
                  moved.begin() + base + where[k] * node_words);
    for (uint32_t &w : moved)
        if ((w >> 30) == 2u) w = 0x80000000u | where[w & 0xffffffu];  // split markers: the child node's new index
    tab.swap(moved);
}

// The per-channel maps of a warped table (see accel_scan_warp_kernel).
struct WarpMaps {
    uint8_t lut[3][256];  // colour value -> warped coordinate
    int lo[3][257];       // lo[c][u]: the smallest value whose warped coordinate is >= u (256 when there is none)
};

// 16 cells per channel, cell i starting at the palette's coordinate of rank K*i/16 (boundaries kept strictly
// increasing); inside a cell of w values, value number k sits at sub-position k*16/w.
inline void make_warp(const std::vector<uint32_t> &coord4, WarpMaps &wm)
{
    const size_t K = coord4.size();
    for (int c = 0; c < 3; ++c) {
        std::vector<int> v(K);
        for (size_t j = 0; j < K; ++j) v[j] = (coord4[j] >> (8 * c)) & 255;
        std::sort(v.begin(), v.end());
        int a[17];
        a[0] = 0;
        a[16] = 256;
        for (int i = 1; i < 16; ++i) {
            int q = v[K * (size_t)i / 16];
            q = std::max(q, a[i - 1] + 1);
            q = std::min(q, 256 - (16 - i));
            a[i] = q;
        }
        for (int i = 0; i < 16; ++i) {
            const int w = a[i + 1] - a[i];
            for (int x = a[i]; x < a[i + 1]; ++x) wm.lut[c][x] = (uint8_t)(16 * i + ((x - a[i]) * 16) / w);
        }
        int x = 0;
        for (int u = 0; u <= 256; ++u) {
            while (x < 256 && (int)wm.lut[c][x] < u) ++x;
            wm.lo[c][u] = x;
        }
    }
}

// the palette entries and, for each entry, the points a quarter and half of the way to its four nearest other entries
inline std::vector<uint32_t> mass_points(const std::vector<uint32_t> &coord4)
{
    std::vector<uint32_t> out(coord4);
    const size_t K = coord4.size();
    constexpr int kNear = 4;
    for (size_t j = 0; j < K && K > (size_t)kNear; ++j) {
        const int r = coord4[j] & 255, g = (coord4[j] >> 8) & 255, b = (coord4[j] >> 16) & 255;
        uint64_t best[kNear];
        for (uint64_t &v : best) v = ~0ull;
        for (size_t k = 0; k < K; ++k) {
            if (k == j) continue;
            const int dr = (int)(coord4[k] & 255) - r, dg = (int)((coord4[k] >> 8) & 255) - g, db = (int)((coord4[k] >> 16) & 255) - b;
            uint64_t key = ((uint64_t)(dr * dr + dg * dg + db * db) << 32) | k;
            for (uint64_t &v : best)
                if (key < v) std::swap(key, v);
        }
        for (const uint64_t key : best) {
            const uint32_t c = coord4[key & 0xffffffffu];
            const int cr = c & 255, cg = (c >> 8) & 255, cb = (c >> 16) & 255;
            for (const int q : {1, 2})  // quarters of the way
                out.push_back((uint32_t)(r + (cr - r) * q / 4) | ((uint32_t)(g + (cg - g) * q / 4) << 8) | ((uint32_t)(b + (cb - b) * q / 4) << 16));
        }
    }
    return out;
}

// One byte per entry: the table `tab` of 8-entry blocks (4096 cell blocks, then 8 blocks per split node; entries = packed
// colours in palette-index order, a block whose first word has bit 31 set = marker) with every colour replaced by the
// index of its palette entry, two words per block.  Entries of equal colour (duplicated palette entries) get their indices
// in ascending order, as the index-ordered block has them.  Marker blocks become {marker, 0xffffffff} with the marker
// 0x80000000 | byte offset of the node's eight blocks in THIS table (split) or 0xC0000000 (too many candidates).
constexpr int kCompactMaxWords = 36 * 1024;  // 144 KB: what ordered_compact_kernel can hold next to records, maps, thresholds
inline std::vector<uint32_t> compact_table(const std::vector<uint32_t> &tab, const std::vector<uint32_t> &coord4)
{
    std::vector<std::pair<uint32_t, uint32_t>> by_colour(coord4.size());
    for (size_t j = 0; j < coord4.size(); ++j) by_colour[j] = {coord4[j], (uint32_t)j};
    std::sort(by_colour.begin(), by_colour.end());  // ascending index among equal colours
    std::vector<uint32_t> out(tab.size() / 4);
    for (size_t b = 0; b + 8 <= tab.size(); b += 8) {
        if (tab[b] >> 31) {
            const bool split = (tab[b] >> 30) == 2u;
            out[b / 4] = split ? (0x80000000u | (uint32_t)((4096u + (tab[b] & 0xffffffu) * 8u) * 8u)) : 0xC0000000u;
            out[b / 4 + 1] = 0xffffffffu;
            continue;
        }
        uint32_t w[2] = {0u, 0u};
        for (int i = 0; i < 8; ++i) {
            int nth = 0;  // how many earlier entries of the block have this colour
            for (int k = 0; k < i; ++k) nth += tab[b + k] == tab[b + i];
            auto it = std::lower_bound(by_colour.begin(), by_colour.end(), std::make_pair(tab[b + i], 0u));
            uint32_t idx = 0u;
            if (it != by_colour.end() && it->first == tab[b + i]) {
                if ((size_t)(it - by_colour.begin()) + nth < by_colour.size() && (it + nth)->first == tab[b + i]) it += nth;
                idx = it->second;
            }
            w[i >> 2] |= idx << (8 * (i & 3));
        }
        out[b / 4] = w[0];
        out[b / 4 + 1] = w[1];
    }
    return out;
}

// how many of the given points (coordinates as the table sees them) sit in split cells
inline int entries_in_split_cells(const std::vector<uint32_t> &tab, const int bw, const std::vector<uint32_t> &coord4)
{
    int n = 0;
    for (const uint32_t c : coord4) {
        const size_t slot = (size_t)cell_slot((c & 255) >> 4, ((c >> 8) & 255) >> 4, ((c >> 16) & 255) >> 4);
        n += (int)(tab[slot * bw] >> 31);
    }
    return n;
}


// ---------------------------------------------------------------------------------------------
// The fine table of ordered_fine_kernel (ordered.hip): candidate WINDOWS shared by the 32^3 cells of 8 colours a side.
//
// On 8-wide cells the sets are short -- palr(256,7): a nearest set N above 4 entries in 0.8 % of the cells, a set T (everything
// up to the second distance) above 6 in 0.5 % -- so a nearest-only slot of the kernel ranks 4 candidates and a full slot 6.  A
// direct table (32768 x 24 bytes) does not fit LDS, but a block may hold ANY real entry besides the cell's own (see make_block),
// so many cells share one block: a window is a quad A of four and a pair B of two palette entries, six distinct ones, and
// serves every cell with N inside A and T inside A + B.  Cells whose sets are longer are WIDE: they map to the reserved window
// 0 (six times entry 0: its keys tie, so the kernel defers the pixel without a test of its own) and their whole T sits in a
// flat list of kWideList entries in index order, as for the split cells of the fast kernel.
// Cells are numbered r>>3 | (g>>3)<<5 | (b>>3)<<10.
// ---------------------------------------------------------------------------------------------
constexpr int kFineCells = 32 * 32 * 32;
constexpr int kFineQuad = 4, kFineWindow = 6;  // entries of A, of A + B
constexpr int kFineIds = kWideCap;             // the ascending cell numbers of the wide cells, padded to this many with 0xffff

inline int fine_cell(const int r, const int g, const int b) { return (r >> 3) | ((g >> 3) << 5) | ((b >> 3) << 10); }
// The two-level table: a wide cell's eight sub-cells of 4 colours a side, numbered by bit 2 of r, g and b, have sets of their own,
// and all but a few of them fit a window.  The cell's entry of `off` is then this tag plus the cell's rank among the wide cells (read
// as int16 it is negative: one compare), and row `rank` holds the windows of the eight sub-cells.
constexpr uint16_t kFineSubTag = 0x8000u;
inline int fine_sub_cell(const int r, const int g, const int b) { return ((r >> 2) & 1) | (((g >> 2) & 1) << 1) | (((b >> 2) & 1) << 2); }

struct FineTable {
    bool ok = false;             // false: no fine table for this palette (a set above kWideList, too many wide cells or windows)
    int n_win = 0, n_wide = 0;   // windows (the reserved one included), wide cells
    std::vector<uint16_t> off;   // [kFineCells] the window of the cell; 0: a wide cell
    std::vector<uint32_t> quad;  // [n_win][4] A: packed colours
    std::vector<uint32_t> pair;  // [n_win][2] B
    std::vector<uint16_t> win_idx;   // [n_win][6] the same entries as palette indices
    std::vector<uint16_t> wide_cell; // [n_wide] ascending
    std::vector<uint32_t> wide;      // [n_wide][kWideList] T(cell) in index order, padded with further entries
    std::vector<uint16_t> wide_idx;  // ... as palette indices
    // the two-level table (fine_pack_sub): off[wide cell] = kFineSubTag | its rank among the wide cells, and a row per wide cell
    bool sub = false;
    std::vector<uint16_t> rows;      // [n_wide][8] the window of each 4-wide sub-cell; 0 (the reserved window): still wide
    std::vector<uint16_t> sub_wide;  // rank * 8 + sub-cell of the still-wide sub-cells, ascending
    // the image the kernel copies to LDS: A | wide lists | B | off (two per word) | wide cell numbers (kFineIds, two per word)
    std::vector<uint32_t> lds_image() const
    {
        std::vector<uint32_t> im;
        im.reserve(quad.size() + wide.size() + pair.size() + kFineCells / 2 + kFineIds / 2);
        im.insert(im.end(), quad.begin(), quad.end());
        im.insert(im.end(), wide.begin(), wide.end());
        im.insert(im.end(), pair.begin(), pair.end());
        for (int c = 0; c < kFineCells; c += 2) im.push_back((uint32_t)off[c] | ((uint32_t)off[c + 1] << 16));
        for (int i = 0; i < kFineIds; i += 2) {
            const uint32_t lo = i < n_wide ? wide_cell[i] : 0xffffu, hi = i + 1 < n_wide ? wide_cell[i + 1] : 0xffffu;
            im.push_back(lo | (hi << 16));
        }
        return im;
    }
    // the image of the two-level table: A | wide lists | B | off with tags (two per word) | rows (two entries per word)
    std::vector<uint32_t> sub_image() const
    {
        std::vector<uint32_t> im;
        im.reserve(quad.size() + wide.size() + pair.size() + kFineCells / 2 + rows.size() / 2);
        im.insert(im.end(), quad.begin(), quad.end());
        im.insert(im.end(), wide.begin(), wide.end());
        im.insert(im.end(), pair.begin(), pair.end());
        for (int c = 0; c < kFineCells; c += 2) im.push_back((uint32_t)off[c] | ((uint32_t)off[c + 1] << 16));
        for (size_t i = 0; i < rows.size(); i += 2) im.push_back((uint32_t)rows[i] | ((uint32_t)rows[i + 1] << 16));
        return im;
    }
};

// tmask / nmask: [kFineCells][mw] membership of T(cell) / N(cell), cells numbered by fine_cell.  fits(n_win, n_wide): whether
// the caller's LDS budget admits a table of that size (ordered_fine.h).  Deterministic and single-threaded: the cells are taken
// longest T first, then longest N, then by number; a cell whose pair (N, T) was met before takes that cell's window; any other
// goes into the window -- among those that hold its rarest member of N in their quad -- that needs the fewest new entries (the
// lowest numbered among equals), or into a new window when none takes it.  Sets are 256-bit masks throughout (K <= 256).
// fine_pack_units is both packers: `sub` false is fine_pack; true is fine_pack_sub, which computes the sets of the sub-cells of the
// wide cells from the cells' flat lists (N(x) and T(x) of a colour lie inside T(cell)) and packs the cells that are not wide and the
// sub-cells that are not wide as ONE population under the same rule: a unit is a cell (its number) or a sub-cell (kFineCells + 8 *
// rank + sub-cell), ordered longest T first, then longest N, then by unit number.  fits(n_win, n_wide) is then the budget of the
// two-level layout (ordered_fine.h: fine_sub_fits).
template <class Fits>
void fine_pack_units(const uint32_t *tmask, const uint32_t *nmask, const int mw, const int K, const std::vector<uint32_t> &coord4, Fits fits,
                     FineTable &ft, const bool sub)
{
    ft = FineTable{};
    if (K < kWideList || K > 256 || K > 32 * mw) return;
    struct Mask {
        uint64_t w[4];
        int count() const  // (a handful of members: clearing them one by one beats a population count without hardware support)
        {
            int n = 0;
            for (int i = 0; i < 4; ++i)
                for (uint64_t bits = w[i]; bits; bits &= bits - 1ull) ++n;
            return n;
        }
        bool any() const { return (w[0] | w[1] | w[2] | w[3]) != 0; }
        bool operator==(const Mask &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
        Mask without(const Mask &o) const { return Mask{{w[0] & ~o.w[0], w[1] & ~o.w[1], w[2] & ~o.w[2], w[3] & ~o.w[3]}}; }
        Mask with(const Mask &o) const { return Mask{{w[0] | o.w[0], w[1] | o.w[1], w[2] | o.w[2], w[3] | o.w[3]}}; }
        void set(const int j) { w[j >> 6] |= 1ull << (j & 63); }
    };
    auto load = [&](const uint32_t *m) {  // the members below K
        Mask r{{0, 0, 0, 0}};
        for (int wi = 0; wi < mw && wi < 8; ++wi) r.w[wi >> 1] |= (uint64_t)m[wi] << (32 * (wi & 1));
        for (int j = K; j < 256; ++j) r.w[j >> 6] &= ~(1ull << (j & 63));
        return r;
    };
    // calls f(j) for the members in ascending order
    auto each = [](const Mask &m, auto f) {
        for (int wi = 0; wi < 4; ++wi)
            for (uint64_t bits = m.w[wi]; bits; bits &= bits - 1ull) f(64 * wi + __builtin_ctzll(bits));
    };
    ft.off.assign(kFineCells, 0);
    std::vector<Mask> tms(kFineCells), nms(kFineCells);
    constexpr int kClasses = (kFineWindow + 1) * (kFineQuad + 1);
    int class_count[kClasses + 1] = {0};
    std::vector<uint8_t> cls(kFineCells, 0xff);  // 0xff: wide
    for (int cell = 0; cell < kFineCells; ++cell) {
        const Mask tm = tms[cell] = load(tmask + (size_t)cell * mw), nm = nms[cell] = load(nmask + (size_t)cell * mw);
        const int nt = tm.count(), nn = nm.count();
        if (nt > kWideList) return;  // not even a flat list holds it
        if (nn > kFineQuad || nt > kFineWindow) {
            if (ft.n_wide == kFineIds || !fits(1, ft.n_wide + 1)) return;
            ++ft.n_wide;
            ft.wide_cell.push_back((uint16_t)cell);
            // the whole list, padded with the lowest unused indices (any real entry is harmless), in index order
            Mask list = tm;
            for (int j = 0, n = nt; n < kWideList; ++j)
                if (!(tm.w[j >> 6] >> (j & 63) & 1ull)) {
                    list.set(j);
                    ++n;
                }
            each(list, [&](const int j) {
                ft.wide_idx.push_back((uint16_t)j);
                ft.wide.push_back(coord4[j]);
            });
            continue;
        }
        cls[cell] = (uint8_t)((kFineWindow - nt) * (kFineQuad + 1) + (kFineQuad - nn));  // longest T first, then longest N
        ++class_count[cls[cell] + 1];
    }
    const int n_units = kFineCells + (sub ? 8 * ft.n_wide : 0);
    if (sub) {
        tms.resize(n_units), nms.resize(n_units), cls.resize(n_units, 0xff);
        for (int k = 0; k < ft.n_wide; ++k) {
            const int cell = ft.wide_cell[k];
            const int r0 = (cell & 31) * 8, g0 = ((cell >> 5) & 31) * 8, b0 = (cell >> 10) * 8;
            const uint16_t *list = &ft.wide_idx[(size_t)k * kWideList];
            int pr[kWideList], pg[kWideList], pb[kWideList];
            for (int i = 0; i < kWideList; ++i) {
                const uint32_t c = coord4[list[i]];
                pr[i] = (int)(c & 255u), pg[i] = (int)((c >> 8) & 255u), pb[i] = (int)((c >> 16) & 255u);
            }
            for (int s = 0; s < 8; ++s) {
                Mask tm{{0, 0, 0, 0}}, nm{{0, 0, 0, 0}};
                for (int i = 0; i < 64; ++i) {
                    const int r = r0 + (s & 1) * 4 + (i & 3), g = g0 + ((s >> 1) & 1) * 4 + ((i >> 2) & 3), b = b0 + (s >> 2) * 4 + (i >> 4);
                    int d[kWideList], d0 = 1 << 30, d1 = 1 << 30;  // the two smallest, with multiplicity
                    for (int q = 0; q < kWideList; ++q) {
                        d[q] = (r - pr[q]) * (r - pr[q]) + (g - pg[q]) * (g - pg[q]) + (b - pb[q]) * (b - pb[q]);
                        if (d[q] < d0) d1 = d0, d0 = d[q];
                        else if (d[q] < d1) d1 = d[q];
                    }
                    for (int q = 0; q < kWideList; ++q) {
                        if (d[q] <= d1) tm.set(list[q]);
                        if (d[q] == d0) nm.set(list[q]);
                    }
                }
                const int u = kFineCells + 8 * k + s;
                tms[u] = tm, nms[u] = nm;
                const int nt = tm.count(), nn = nm.count();
                if (nn > kFineQuad || nt > kFineWindow) {
                    ft.sub_wide.push_back((uint16_t)(8 * k + s));
                    continue;
                }
                cls[u] = (uint8_t)((kFineWindow - nt) * (kFineQuad + 1) + (kFineQuad - nn));
                ++class_count[cls[u] + 1];
            }
        }
    }
    for (int c = 0; c < kClasses; ++c) class_count[c + 1] += class_count[c];
    std::vector<int> order(class_count[kClasses]);
    for (int cell = 0; cell < n_units; ++cell)
        if (cls[cell] != 0xff) order[class_count[cls[cell]]++] = cell;
    std::vector<uint16_t> unit_win(sub ? n_units : 0, 0);  // (the cells' are ft.off)
    auto win_of = [&](const int u) -> uint16_t & { return u < kFineCells ? ft.off[u] : unit_win[u]; };
    struct Win {
        Mask a, ab;  // the quad, the whole window
        int na, nb;
    };
    std::vector<Win> wins(1, Win{Mask{{0, 0, 0, 0}}, Mask{{0, 0, 0, 0}}, kFineQuad, kFineWindow - kFineQuad});  // (window 0: reserved)
    std::vector<std::vector<int>> holds(K);       // entry -> the windows that hold it in their quad
    constexpr int kSlots = 1 << 16;               // the pairs met so far: open addressing, cell number + 1
    std::vector<int> seen(kSlots, 0);
    for (const int cell : order) {
        const Mask &nm = nms[cell], &tm = tms[cell];
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (int wi = 0; wi < 4; ++wi) h = (h ^ nm.w[wi]) * 0xff51afd7ed558ccdull, h = (h ^ (h >> 29) ^ tm.w[wi]) * 0xc4ceb9fe1a85ec53ull;
        int slot = (int)((h >> 40) & (kSlots - 1));
        bool met = false;
        for (; seen[slot] != 0; slot = (slot + 1) & (kSlots - 1))
            if (nms[seen[slot] - 1] == nm && tms[seen[slot] - 1] == tm) {
                win_of(cell) = win_of(seen[slot] - 1);
                met = true;
                break;
            }
        if (met) continue;
        seen[slot] = cell + 1;
        const Mask rest = tm.without(nm);
        int best = -1, best_cost = kFineWindow + 1;
        // (the windows that hold the member of N with the fewest windows: every window that holds all of N is among them)
        int rarest = -1;
        each(nm, [&](const int j) {
            if (rarest < 0 || holds[j].size() < holds[rarest].size()) rarest = j;
        });
        {
            for (const int wi : holds[rarest]) {
                const Win &w = wins[wi];
                // what the window would need: nothing of N may sit in its pair, N must find room in the quad, the rest anywhere
                const Mask need_a = nm.without(w.a), need_r = rest.without(w.ab);
                int c = 0;
                if (need_a.any() || need_r.any()) {
                    if (w.na + w.nb == kFineWindow || need_a.without(w.ab).w[0] != need_a.w[0] || need_a.without(w.ab).w[1] != need_a.w[1] ||
                        need_a.without(w.ab).w[2] != need_a.w[2] || need_a.without(w.ab).w[3] != need_a.w[3])
                        continue;
                    const int add_a = need_a.count();
                    if (w.na + add_a > kFineQuad) continue;
                    const int add_r = need_r.count();
                    if (add_r > (kFineQuad - w.na - add_a) + (kFineWindow - kFineQuad - w.nb)) continue;
                    c = add_a + add_r;
                }
                if (c < best_cost || (c == best_cost && wi < best)) {
                    best = wi;
                    best_cost = c;
                }
            }
        }
        if (best < 0) {
            if (wins.size() == 0xffffu || !fits((int)wins.size() + 1, ft.n_wide)) return;
            best = (int)wins.size();
            wins.push_back(Win{Mask{{0, 0, 0, 0}}, Mask{{0, 0, 0, 0}}, 0, 0});
        }
        Win &w = wins[best];
        each(nm.without(w.a), [&](const int j) {
            w.a.set(j);
            w.ab.set(j);
            ++w.na;
            holds[j].push_back(best);
        });
        each(rest.without(w.ab), [&](const int j) {  // the rest of T: into the pair while it has room (the quad's places are the scarce ones)
            w.ab.set(j);
            if (w.nb < kFineWindow - kFineQuad) {
                ++w.nb;
            } else {
                w.a.set(j);
                ++w.na;
                holds[j].push_back(best);
            }
        });
        win_of(cell) = (uint16_t)best;
    }
    if (sub) {
        ft.sub = true;
        ft.rows.assign(unit_win.begin() + kFineCells, unit_win.end());
        for (int k = 0; k < ft.n_wide; ++k) ft.off[ft.wide_cell[k]] = (uint16_t)(kFineSubTag | k);
    }
    // free places: the lowest indices the window does not hold yet; the reserved window: entry 0 six times
    ft.n_win = (int)wins.size();
    ft.win_idx.assign((size_t)ft.n_win * kFineWindow, 0);
    for (int wi = 1; wi < ft.n_win; ++wi) {
        Win &w = wins[wi];
        for (int j = 0; w.na + w.nb < kFineWindow; ++j)
            if (!(w.ab.w[j >> 6] >> (j & 63) & 1ull)) {
                w.ab.set(j);
                if (w.na < kFineQuad) w.a.set(j), ++w.na;
                else ++w.nb;
            }
        uint16_t *e = &ft.win_idx[(size_t)wi * kFineWindow];
        int pa = 0, pb = kFineQuad;
        each(w.a, [&](const int j) { e[pa++] = (uint16_t)j; });
        each(w.ab.without(w.a), [&](const int j) { e[pb++] = (uint16_t)j; });
    }
    ft.quad.resize((size_t)ft.n_win * kFineQuad);
    ft.pair.resize((size_t)ft.n_win * (kFineWindow - kFineQuad));
    for (int wi = 0; wi < ft.n_win; ++wi)
        for (int p = 0; p < kFineWindow; ++p) {
            const uint32_t c = coord4[ft.win_idx[(size_t)wi * kFineWindow + p]];
            if (p < kFineQuad) ft.quad[(size_t)wi * kFineQuad + p] = c;
            else ft.pair[(size_t)wi * (kFineWindow - kFineQuad) + p - kFineQuad] = c;
        }
    ft.ok = true;
}

// Today's table: the cells alone.  Its output is what tests/test_ordered_fine_cpu.py checks and does not depend on the other packer.
template <class Fits>
void fine_pack(const uint32_t *tmask, const uint32_t *nmask, const int mw, const int K, const std::vector<uint32_t> &coord4, Fits fits,
               FineTable &ft)
{
    fine_pack_units(tmask, nmask, mw, K, coord4, fits, ft, false);
}
// The two-level table: cells and the sub-cells of the wide cells packed together (see fine_pack_units).
template <class Fits>
void fine_pack_sub(const uint32_t *tmask, const uint32_t *nmask, const int mw, const int K, const std::vector<uint32_t> &coord4, Fits fits,
                   FineTable &ft)
{
    fine_pack_units(tmask, nmask, mw, K, coord4, fits, ft, true);
}


// ---------------------------------------------------------------------------------------------
// Median cut as the reference runs it (ColorReducer.reduce_colors, dithering_lib.py:1813-1843):
//     median_cut(list(set(image.getdata())), depth)
// The cut sorts stably, so the ITERATION ORDER OF THE PYTHON SET is observable in the palette.  That order is a pure
// function of the insertion sequence: CPython's tuple hash (xxHash-style, Objects/tupleobject.c, 3.8+; small ints hash to
// themselves) and the open-addressing table of Objects/setobject.c (linear probes of 9 + perturbed jumps, growth to
// used*4 -- used*2 above 50 000 -- whenever fill*5 >= mask*3, re-insertion in slot order).  pyset_order() replays it and
// returns the elements in the order `list(set(...))` yields them, without creating a Python object per colour (1.2 M
// tuples of a 4K photograph: ~1 s of interpreter time).  The Python side checks the replay against the running
// interpreter's own set once per process and keeps building real sets if they ever disagree.
// ---------------------------------------------------------------------------------------------
inline uint64_t py_tuple3_hash(const uint64_t a, const uint64_t b, const uint64_t c)
{
    constexpr uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P5 = 2870177450012600261ULL;
    uint64_t acc = P5;
    for (const uint64_t lane : {a, b, c}) {
        acc += lane * P2;
        acc = (acc << 31) | (acc >> 33);
        acc *= P1;
    }
    acc += 3ULL ^ (P5 ^ 3527539ULL);
    return acc == ~0ULL ? 1546275796ULL : acc;
}

// rgb: n colours (3 bytes each) in insertion order, duplicates allowed.  order: for every element of the resulting set, in
// the set's iteration order, the index of its first occurrence in rgb.
// An 8-byte slot {low 32 bits of the hash, index + 1}: the home slot and the duplicate test need no more (tables have fewer than
// 2^32 slots; equal low words are settled by comparing the colours), and the high bits only enter the perturbed jumps after nine
// occupied neighbours, where the hash is simply recomputed from the colour.  Half the table (4 MB instead of 8 for 180 k
// colours) is half the cache misses.  (Prefetching home slots ahead was measured on the bench box's EPYC 9575F and costs time:
// 4.8 -> 6.1 ms, profiles/experiments/r04_pyset_prefetch_ab.txt.)
struct PySetSlot {
    uint32_t h;     // low word of the hash
    uint32_t idx1;  // index of the colour + 1 (0 = unused slot)
};

// Two slot arrays per thread, kept from call to call (a 180 k-colour set walks through 8 MB of tables; fresh allocations cost
// more in page faults than the insertions themselves).  A buffer is handed out zeroed over the slots the caller asks for:
// only what an earlier table left dirty is cleared.
struct PySetTables {
    std::vector<PySetSlot> buf[2];
    size_t dirty[2] = {0, 0};   // slots of each buffer that may be non-zero
    PySetSlot *fresh(const int which, const size_t size)
    {
        if (buf[which].size() < size) {
            buf[which].assign(size, PySetSlot{0, 0});
        } else if (dirty[which]) {
            std::memset(buf[which].data(), 0, std::min(dirty[which], buf[which].size()) * sizeof(PySetSlot));
        }
        dirty[which] = size;
        return buf[which].data();
    }
    void trim()   // (a one-off giant image must not pin hundreds of megabytes for the life of the thread)
    {
        for (int w = 0; w < 2; ++w)
            if (buf[w].size() > ((size_t)1 << 23)) {
                std::vector<PySetSlot>().swap(buf[w]);
                dirty[w] = 0;
            }
    }
};

inline void pyset_order(const uint8_t *rgb, const size_t n, std::vector<uint32_t> &order)
{
    constexpr size_t kLinearProbes = 9;
    constexpr int kPerturbShift = 5;
    order.clear();
    static thread_local PySetTables tables;
    size_t mask = 7, fill = 0;
    int cur = 0;
    PySetSlot *tab = tables.fresh(0, 8);
    auto hash_of = [&](const size_t k) { return py_tuple3_hash(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2]); };
    auto same = [&](const uint32_t slot_idx, const size_t k) {
        const uint8_t *p = rgb + 3 * (size_t)(slot_idx - 1), *q = rgb + 3 * k;
        return p[0] == q[0] && p[1] == q[1] && p[2] == q[2];
    };
    // insertion of an element that is known to be absent (growth steps)
    auto insert_clean = [&](PySetSlot *nt, const size_t m, const uint32_t hlo, const uint32_t idx1) {
        size_t i = (size_t)hlo & m;
        if (nt[i].idx1 == 0) {
            nt[i] = PySetSlot{hlo, idx1};
            return;
        }
        uint64_t perturb = 0;
        bool have_hash = false;
        for (;;) {
            if (i + kLinearProbes <= m)
                for (size_t j = 1; j <= kLinearProbes; ++j)
                    if (nt[i + j].idx1 == 0) {
                        nt[i + j] = PySetSlot{hlo, idx1};
                        return;
                    }
            if (!have_hash) {
                perturb = hash_of((size_t)idx1 - 1);
                have_hash = true;
            }
            perturb >>= kPerturbShift;
            i = (i * 5 + 1 + (size_t)perturb) & m;
            if (nt[i].idx1 == 0) {
                nt[i] = PySetSlot{hlo, idx1};
                return;
            }
        }
    };
    for (size_t k = 0; k < n; ++k) {
        const uint64_t h = hash_of(k);
        const uint32_t hlo = (uint32_t)h;
        uint64_t perturb = h;
        size_t i = (size_t)h & mask;
        bool added = false;
        for (bool done = false; !done;) {
            size_t probes = i + kLinearProbes <= mask ? kLinearProbes : 0;
            for (size_t j = i;; ++j) {
                if (tab[j].idx1 == 0) {
                    tab[j] = PySetSlot{hlo, (uint32_t)k + 1u};
                    added = done = true;
                    break;
                }
                if (tab[j].h == hlo && same(tab[j].idx1, k)) {
                    done = true;  // already in the set
                    break;
                }
                if (probes == 0) break;
                --probes;
            }
            if (!done) {
                perturb >>= kPerturbShift;
                i = (i * 5 + 1 + (size_t)perturb) & mask;
            }
        }
        if (added && ++fill * 5 >= mask * 3) {
            const size_t minused = fill > 50000 ? fill * 2 : fill * 4;  // (no deletions: used == fill)
            size_t newsize = 8;
            while (newsize <= minused) newsize <<= 1;
            PySetSlot *nt = tables.fresh(cur ^ 1, newsize);
            const size_t m = newsize - 1;
            for (size_t slot = 0; slot <= mask; ++slot)   // re-insertion in slot order (the old table is read sequentially)
                if (tab[slot].idx1 != 0) insert_clean(nt, m, tab[slot].h, tab[slot].idx1);
            tab = nt;
            cur ^= 1;
            mask = m;
        }
    }
    order.reserve(fill);
    for (size_t slot = 0; slot <= mask; ++slot)
        if (tab[slot].idx1 != 0) order.push_back(tab[slot].idx1 - 1u);
    tables.trim();
}

// median_cut(colors, depth) of the reference (dithering_lib.py:1822-1833) on n colours in list order: the first widest
// channel, a STABLE sort on it (a counting sort over the 256 values), split at n // 2, at depth 0 the per-channel mean
// int(sum / n) (true division in float64, truncated); an empty bucket yields the single entry (0, 0, 0) at any depth.
// The colours travel as packed words r | g << 8 | b << 16 between two buffers (cur -> other at every level: no copy back);
// the palette entries are appended to out (3 ints each).
// threads > 1: the two halves of a big bucket are cut concurrently (they work on disjoint parts of both buffers; the left
// half's entries come first in the palette, as in the recursion).
inline void median_cut_u32(uint32_t *cur, uint32_t *other, const size_t n, const int depth, std::vector<int32_t> &out, const int threads = 1)
{
    if (n == 0) {
        out.insert(out.end(), {0, 0, 0});
        return;
    }
    if (depth == 0) {
        uint64_t s0 = 0, s1 = 0, s2 = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t v = cur[i];
            s0 += v & 255u;
            s1 += (v >> 8) & 255u;
            s2 += v >> 16;
        }
        out.push_back((int32_t)((double)s0 / (double)n));
        out.push_back((int32_t)((double)s1 / (double)n));
        out.push_back((int32_t)((double)s2 / (double)n));
        return;
    }
    // per-channel minimum and maximum, all three at once on the packed word (byte-wise min / max: the compiler vectorises it)
    uint8_t lo[4] = {255, 255, 255, 255}, hi[4] = {0, 0, 0, 0};
    {
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(cur);
        uint8_t l0 = 255, l1 = 255, l2 = 255, h0 = 0, h1 = 0, h2 = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t a = bytes[4 * i], b = bytes[4 * i + 1], c = bytes[4 * i + 2];
            l0 = a < l0 ? a : l0;
            h0 = a > h0 ? a : h0;
            l1 = b < l1 ? b : l1;
            h1 = b > h1 ? b : h1;
            l2 = c < l2 ? c : l2;
            h2 = c > h2 ? c : h2;
        }
        lo[0] = l0; lo[1] = l1; lo[2] = l2;
        hi[0] = h0; hi[1] = h1; hi[2] = h2;
    }
    int ch = 0;
    for (int c = 1; c < 3; ++c)
        if (hi[c] - lo[c] > hi[ch] - lo[ch]) ch = c;  // the first of equal spans
    const int sh = 8 * ch;
    size_t start[257] = {0};
    for (size_t i = 0; i < n; ++i) ++start[((cur[i] >> sh) & 255u) + 1];
    for (int v = 0; v < 256; ++v) start[v + 1] += start[v];
    for (size_t i = 0; i < n; ++i) other[start[(cur[i] >> sh) & 255u]++] = cur[i];
    const size_t half = n / 2;
    if (threads > 1 && n >= 16384) {
        // (an exception -- bad_alloc while `right` or `out` grows -- must neither leave the lambda, which would call
        // std::terminate, nor destroy `t` while it is joinable, which would too: it is carried across the join and rethrown)
        std::vector<int32_t> right;
        std::exception_ptr failed;
        std::thread t([&] {
            try {
                median_cut_u32(other + half, cur + half, n - half, depth - 1, right, threads / 2);
            } catch (...) {
                failed = std::current_exception();
            }
        });
        struct Joiner {
            std::thread &t;
            ~Joiner() { if (t.joinable()) t.join(); }
        } joiner{t};
        median_cut_u32(other, cur, half, depth - 1, out, threads - threads / 2);
        t.join();
        if (failed) std::rethrow_exception(failed);
        out.insert(out.end(), right.begin(), right.end());
        return;
    }
    median_cut_u32(other, cur, half, depth - 1, out, 1);
    median_cut_u32(other + half, cur + half, n - half, depth - 1, out, 1);
}

// ---- colour -> palette index map (indexed.hip, include/ditherpie_hip_indexed.h) ---------------------------------------
// An open-addressing table the index kernels keep in LDS.  A colour c = r | g << 8 | b << 16 is hashed by
// h = (c * mult) mod 2^24 with an odd mult, a BIJECTION of the 24-bit colours, so (home slot, rest) = (h >> rest_bits,
// h & rest_mask) names the colour and a four-byte slot has room for the index beside it:
//   bits 0..12   rest  (13 bits at 2048 slots, 12 at 4096)
//   bits 13..15  disp  slots between the entry's home and where linear probing put it, 0..kIndexMapMaxProbe
//   bits 16..25  index (the LOWEST j with C[j] == c: colours are inserted in index order, later duplicates are dropped)
// 0xFFFFFFFF is an empty slot (disp 7 is never stored).  A reader at step d of its probe run compares the low 16 bits of
// slot (home + d) mod slots with rest | d << 13: equal rest and equal disp mean equal home, hence equal h, hence the same
// colour -- no second table, no false positive, and no need to stop at an empty slot: the run is bounded by the map's own
// longest displacement, which the builder keeps <= kIndexMapMaxProbe by choosing mult.
constexpr int kIndexMapMaxProbe = 6;        // the kernels are compiled for at most this displacement (7 probes)
constexpr int kIndexMapMaxSlots = 4096;
constexpr uint32_t kIndexMapEmpty = 0xFFFFFFFFu;

struct IndexMapHost {
    int K = 0;
    int slots = 0;        // 2048 for K <= 512, 4096 above: the load never exceeds 1/4
    int rest_bits = 0;    // 24 - log2(slots)
    int max_probe = 0;    // longest displacement of any entry
    uint32_t mult = 0;
    std::vector<uint32_t> table;   // slots words
    std::vector<uint32_t> colors;  // K: r | g << 8 | b << 16 (what an index decodes to)
};

inline uint32_t index_map_hash(const uint32_t c, const uint32_t mult) { return (c * mult) & 0xFFFFFFu; }

// index of colour c, or -1 when no entry equals it: what the kernels compute, restated for the host
inline int index_map_lookup(const IndexMapHost &m, const uint32_t c)
{
    const uint32_t h = index_map_hash(c, m.mult), home = h >> m.rest_bits, rest = h & ((1u << m.rest_bits) - 1u);
    for (int d = 0; d <= m.max_probe; ++d) {
        const uint32_t w = m.table[(home + (uint32_t)d) & (uint32_t)(m.slots - 1)];
        if ((w & 0xFFFFu) == (rest | ((uint32_t)d << 13))) return (int)(w >> 16);
    }
    return -1;
}

// Fills `table` for one multiplier; returns the longest displacement, or -1 when an entry would need more than `limit`.
inline int index_map_fill(const std::vector<uint32_t> &colors, const int slots, const int rest_bits, const uint32_t mult,
                          const int limit, std::vector<uint32_t> &table)
{
    table.assign((size_t)slots, kIndexMapEmpty);
    const uint32_t mask = (uint32_t)slots - 1u, rest_mask = (1u << rest_bits) - 1u;
    int longest = 0;
    for (size_t j = 0; j < colors.size(); ++j) {
        const uint32_t h = index_map_hash(colors[j], mult), home = h >> rest_bits, rest = h & rest_mask;
        int d = 0;
        for (;; ++d) {
            if (d > limit) return -1;
            uint32_t &w = table[(home + (uint32_t)d) & mask];
            if (w == kIndexMapEmpty) {
                w = rest | ((uint32_t)d << 13) | ((uint32_t)j << 16);
                break;
            }
            if ((w & 0xFFFFu) == (rest | ((uint32_t)d << 13))) break;   // the colour is there already, at a lower index
        }
        longest = std::max(longest, d);
    }
    return longest;
}

// colors_u8: K x 3 bytes, 1 <= K <= DP_MAX_COLORS (the caller checks).  Tries odd multipliers from a fixed sequence and
// keeps the one with the shortest longest displacement (stopping early at <= 1); false when 4096 candidates all exceed
// kIndexMapMaxProbe (at a load of <= 1/4 the first few candidates succeed on every list tried; the bound is what makes
// the kernels' probe loop finite whatever the list).
inline bool index_map_build(const uint8_t *colors_u8, const int K, IndexMapHost &m)
{
    m.K = K;
    m.slots = K <= 512 ? 2048 : kIndexMapMaxSlots;
    m.rest_bits = K <= 512 ? 13 : 12;
    m.colors.resize((size_t)K);
    for (int j = 0; j < K; ++j)
        m.colors[(size_t)j] = (uint32_t)colors_u8[3 * j] | ((uint32_t)colors_u8[3 * j + 1] << 8) | ((uint32_t)colors_u8[3 * j + 2] << 16);
    std::vector<uint32_t> trial;
    int best = -1;
    uint32_t seq = 0x9E3779B1u;
    for (int t = 0; t < 4096; ++t) {
        const uint32_t mult = ((seq >> 8) | 1u) & 0xFFFFFFu;
        seq = seq * 1664525u + 1013904223u;
        const int longest = index_map_fill(m.colors, m.slots, m.rest_bits, mult, best < 0 ? kIndexMapMaxProbe : best - 1, trial);
        if (longest < 0) continue;
        best = longest;
        m.mult = mult;
        m.max_probe = longest;
        m.table.swap(trial);
        if (best <= 1 || (t >= 15 && best <= 3)) break;
    }
    return best >= 0;
}

// ---- GIF image data (gif.hip, include/ditherpie_hip_gif.h) -------------------------------------------------------------
// The normative statement of the chunked LZW stream: the device kernels write the bytes this writes.  The dictionary is the
// open-addressing table the chunk kernel keeps in LDS: a pair (prefix code, pixel) is the 20-bit key code << 8 | pixel, a
// slot holds key << 12 | the code the pair got, 0xFFFFFFFF is an empty slot (no entry has prefix 4095: by the time code 4095
// exists no code is free).  At most 4096 - 6 entries in 8192 slots, so a probe run ends at an empty slot; the loops are
// bounded by the table size all the same.
constexpr int kGifSlots = 8192;
constexpr uint32_t kGifEmpty = 0xFFFFFFFFu;
constexpr int kGifCodesPerClear = 4096 - 258 + 1;   // codes in front of a Clear inside a chunk, at least (min_code_size 8)

inline uint32_t gif_slot_of(const uint32_t key) { return (key * 0x9E3779B1u) >> 19; }   // 13 bits

inline int64_t gif_chunks(const int64_t n_px, const int64_t chunk_px) { return (n_px + std::min(chunk_px, n_px) - 1) / std::min(chunk_px, n_px); }

// the worst-case size of one frame's image data (the derivation is in the header); n_px >= 1, chunk_px >= 1
inline uint64_t gif_lzw_bound(const int64_t n_px, const int64_t chunk_px)
{
    const uint64_t codes = (uint64_t)n_px + (uint64_t)n_px / kGifCodesPerClear + (uint64_t)gif_chunks(n_px, chunk_px) + 1u;
    const uint64_t d = (12u * codes + 7u) / 8u;
    return 1u + d + (d + 254u) / 255u + 1u;
}

struct GifBits {
    std::vector<uint8_t> data;
    uint64_t acc = 0;
    int n = 0;
    void put(const uint32_t code, const int width)
    {
        acc |= (uint64_t)code << n;
        n += width;
        for (; n >= 8; n -= 8, acc >>= 8) data.push_back((uint8_t)(acc & 0xFFu));
    }
    void flush()
    {
        if (n > 0) data.push_back((uint8_t)(acc & 0xFFu));
        n = 0;
        acc = 0;
    }
};

// One frame: n_px pixels -> `out` (cleared first): min_code_size byte, sub-blocks, terminator.
inline void gif_lzw_encode(const uint8_t *px, const int64_t n_px, const int min_code_size, int64_t chunk_px, std::vector<uint8_t> &out)
{
    const uint32_t clear = 1u << min_code_size, eoi = clear + 1u, mask = clear - 1u;
    chunk_px = std::min(chunk_px, n_px);
    std::vector<uint32_t> table((size_t)kGifSlots);
    GifBits bits;
    int width = min_code_size + 1;
    for (int64_t at = 0; at < n_px; at += chunk_px) {
        const int64_t n = std::min(chunk_px, n_px - at);
        bits.put(clear, width);
        width = min_code_size + 1;
        uint32_t next = clear + 2u;
        std::fill(table.begin(), table.end(), kGifEmpty);
        uint32_t cur = px[at] & mask;
        for (int64_t i = 1; i < n; ++i) {
            const uint32_t c = px[at + i] & mask, key = (cur << 8) | c;
            uint32_t slot = gif_slot_of(key), found = kGifEmpty;
            for (int probe = 0; probe < kGifSlots; ++probe, slot = (slot + 1u) & (uint32_t)(kGifSlots - 1)) {
                const uint32_t e = table[slot];
                if (e == kGifEmpty) break;
                if ((e >> 12) == key) {
                    found = e & 0xFFFu;
                    break;
                }
            }
            if (found != kGifEmpty) {
                cur = found;
                continue;
            }
            bits.put(cur, width);
            if (next < 4096u) {
                table[slot] = (key << 12) | next;   // (the run ended at an empty slot: the table is never full)
                if (next == (1u << width) && width < 12) ++width;
                ++next;
            } else {
                bits.put(clear, 12);
                width = min_code_size + 1;
                next = clear + 2u;
                std::fill(table.begin(), table.end(), kGifEmpty);
            }
            cur = c;
        }
        bits.put(cur, width);
        if (next < 4096u && next == (1u << width) && width < 12) ++width;   // the decoder's lagging entry
    }
    bits.put(eoi, width);
    bits.flush();
    const std::vector<uint8_t> &d = bits.data;
    out.clear();
    out.reserve(d.size() + d.size() / 255 + 3);
    out.push_back((uint8_t)min_code_size);
    for (size_t a = 0; a < d.size(); a += 255) {
        const size_t len = std::min<size_t>(255, d.size() - a);
        out.push_back((uint8_t)len);
        out.insert(out.end(), d.begin() + (std::ptrdiff_t)a, d.begin() + (std::ptrdiff_t)(a + len));
    }
    out.push_back(0);
}

// ---- PNG-8 image data (png.hip, include/ditherpie_hip_png.h) ------------------------------------------------------------
// The normative statement of the segmented zlib stream of one plane of palette indices: the device kernels write the bytes
// this writes.  The pieces both sides need (the filtered byte at an offset, the trigram hash, the fixed-Huffman bits of a
// token) are single functions compiled for host and device, so the two cannot drift apart in a table.
//
// Filtered bytes (never stored anywhere as a whole): row r is a filter byte 0 and ceil(w * depth / 8) packed bytes, the
// leftmost pixel in the high-order bits, unused low bits of the last byte zero, an index taken & ((1 << depth) - 1).
// Segments of seg_bytes filtered bytes (the last may be shorter) are compressed on their own, each into ONE data block:
//   matcher   the candidate of position p (p + 2 < n) is the largest q < p of the segment with png_hash3 equal; its length
//             is the number of equal bytes, at most min(258, n - p).  Greedy: at p a candidate of length >= 3 is taken and
//             p advances by its length, else the byte is a literal.  The candidate is a function of the bytes alone.
//   type      the smallest of stored and fixed-Huffman in bytes of the whole segment (block, and for every segment but the
//             last the empty stored block 'pad to a byte, 00 00 FF FF' that realigns the stream); a tie goes to stored.
//             png_deflate_encode_dyn (below) adds one dynamic-Huffman block over the same tokens as a third candidate;
//             png_deflate_encode writes stored and fixed blocks only, and its bytes do not change.
// BFINAL is set on the data block of the last segment.  The stream is 78 01, the segments, Adler-32 big-endian.
#if defined(__HIPCC__)
#define DP_HD __host__ __device__
#else
#define DP_HD
#endif

constexpr int kPngSegMin = 256, kPngSegMax = 32768;
constexpr int kPngHashBits = 12;
constexpr uint32_t kPngNoCand = 0xFFFFu;
constexpr uint32_t kAdlerMod = 65521u;
constexpr int kPngStored = 0, kPngFixed = 1, kPngDynamic = 2;   // block types in the order ties are resolved

DP_HD inline uint32_t png_hash3(const uint32_t b0, const uint32_t b1, const uint32_t b2)
{
    return ((b0 | (b1 << 8) | (b2 << 16)) * 0x9E3779B1u) >> (32 - kPngHashBits);
}

DP_HD inline uint32_t png_row_bytes(const int w, const int depth) { return 1u + (uint32_t)(((int64_t)w * depth + 7) / 8); }

inline bool png_geometry_ok(const int h, const int w, const int depth, const int seg_bytes)
{
    if (h < 1 || w < 1 || !(depth == 1 || depth == 2 || depth == 4 || depth == 8) || seg_bytes < kPngSegMin || seg_bytes > kPngSegMax) return false;
    return (int64_t)h * (int64_t)(1 + ((int64_t)w * depth + 7) / 8) < (int64_t(1) << 31);
}
inline int64_t png_filtered_size(const int h, const int w, const int depth) { return (int64_t)h * (int64_t)png_row_bytes(w, depth); }
inline int64_t png_segments(const int64_t F, const int seg_bytes) { const int64_t s = std::min<int64_t>(seg_bytes, F); return (F + s - 1) / s; }
// 2 header + every byte stored (5 bytes of block header per segment) + a 5-byte realigning block per segment + 4 trailer
inline uint64_t png_deflate_bound(const int64_t F, const int seg_bytes) { return 2u + (uint64_t)F + 10u * (uint64_t)png_segments(F, seg_bytes) + 4u; }

// the filtered byte at offset r * row_bytes + c of a plane (c < row_bytes)
DP_HD inline uint32_t png_filtered_byte(const uint8_t *plane, const int w, const int depth, const uint32_t r, const uint32_t c)
{
    if (c == 0) return 0u;
    const uint32_t ppb = 8u / (uint32_t)depth, mask = (1u << depth) - 1u;
    const uint32_t x0 = (c - 1u) * ppb;
    const uint8_t *row = plane + (size_t)r * (size_t)w;
    uint32_t v = 0;
    for (uint32_t k = 0; k < ppb; ++k)   // <= 8
        if (x0 + k < (uint32_t)w) v |= ((uint32_t)row[x0 + k] & mask) << (8u - (uint32_t)depth * (k + 1u));
    return v;
}

struct PngBits {
    uint32_t bits;   // LSB first, as they enter the stream
    int nb;          // <= 31
};

DP_HD inline uint32_t png_rev(const uint32_t code, const int nb)   // Huffman codes enter the stream most significant bit first
{
    uint32_t r = 0;
    for (int i = 0; i < nb; ++i) r |= ((code >> i) & 1u) << (nb - 1 - i);   // nb <= 9
    return r;
}

DP_HD inline PngBits png_fixed_symbol(const uint32_t sym)   // RFC 1951 3.2.6
{
    PngBits t;
    if (sym < 144u) { t.bits = png_rev(0x30u + sym, 8); t.nb = 8; }
    else if (sym < 256u) { t.bits = png_rev(0x190u + (sym - 144u), 9); t.nb = 9; }
    else if (sym < 280u) { t.bits = png_rev(sym - 256u, 7); t.nb = 7; }
    else { t.bits = png_rev(0xC0u + (sym - 280u), 8); t.nb = 8; }
    return t;
}

// length 3 ... 258 -> symbol 257 ... 285, extra bits and their value (RFC 1951 3.2.5, as arithmetic)
DP_HD inline void png_length_code(const int len, uint32_t &sym, int &extra, uint32_t &val)
{
    const uint32_t l = (uint32_t)len - 3u;
    if (len == 258) { sym = 285u; extra = 0; val = 0u; }
    else if (l < 8u) { sym = 257u + l; extra = 0; val = 0u; }
    else {
        const int k = 31 - __builtin_clz(l);
        extra = k - 2;
        sym = 261u + 4u * (uint32_t)extra + ((l >> extra) & 3u);
        val = l & ((1u << extra) - 1u);
    }
}

// distance 1 ... 32768 -> code 0 ... 29, extra bits and their value
DP_HD inline void png_dist_code(const int dist, uint32_t &code, int &extra, uint32_t &val)
{
    const uint32_t d = (uint32_t)dist - 1u;
    if (d < 4u) { code = d; extra = 0; val = 0u; }
    else {
        const int k = 31 - __builtin_clz(d);
        extra = k - 1;
        code = 2u * (uint32_t)k + ((d >> extra) & 1u);
        val = d & ((1u << extra) - 1u);
    }
}

DP_HD inline PngBits png_fixed_literal(const uint32_t byte) { return png_fixed_symbol(byte); }

DP_HD inline PngBits png_fixed_match(const int len, const int dist)   // <= 8 + 5 + 5 + 13 = 31 bits
{
    uint32_t sym, lval, dcode, dval;
    int lextra, dextra;
    png_length_code(len, sym, lextra, lval);
    png_dist_code(dist, dcode, dextra, dval);
    PngBits t = png_fixed_symbol(sym);
    t.bits |= lval << t.nb;
    t.nb += lextra;
    t.bits |= png_rev(dcode, 5) << t.nb;
    t.nb += 5;
    t.bits |= dval << t.nb;
    t.nb += dextra;
    return t;
}

// The bytes of one segment for each block type (n data bytes; `bits` = the block's bits from its 3 header bits up to and
// including end-of-block).  Every segment but the last carries the realigning empty stored block.
DP_HD inline uint32_t png_stored_segment_bytes(const uint32_t n, const bool last) { return 5u + n + (last ? 0u : 5u); }
DP_HD inline uint32_t png_huffman_segment_bytes(const uint64_t bits, const bool last) { return last ? (uint32_t)((bits + 7u) / 8u) : (uint32_t)((bits + 3u + 7u) / 8u) + 4u; }
// the type written: the earliest of the smallest
DP_HD inline int png_segment_choice(const uint32_t stored_bytes, const uint32_t fixed_bytes) { return stored_bytes <= fixed_bytes ? kPngStored : kPngFixed; }

DP_HD inline int png_segment_choice(const uint32_t stored_bytes, const uint32_t fixed_bytes, const uint32_t dynamic_bytes)
{
    const int two = png_segment_choice(stored_bytes, fixed_bytes);
    return dynamic_bytes < (two == kPngStored ? stored_bytes : fixed_bytes) ? kPngDynamic : two;
}

// ---- Dynamic-Huffman blocks (include/ditherpie_hip_png_dyn.h) --------------------------------------------------------------
// One dynamic block (BTYPE 10) over the tokens of a segment is the third candidate of png_segment_choice.  Everything that
// decides a bit is a DP_HD function here, run by the host statement and by the device alike; the device replaces only the
// sort of rule (b) and the sums of the size by wave-parallel ones (png.hip).
//
// Code lengths of an alphabet with counts c[0 .. m) and limit L (15 for literal/length and distance, 7 for the code-length
// alphabet):
//   (a) while fewer than two symbols have a count, the lowest-numbered symbol with count 0 gets count 1
//   (b) the used symbols ascending by (count, symbol): one 32-bit key count << 9 | symbol each (counts <= 2^20)
//   (c) two-queue Huffman merge: the front leaf is taken when its weight is <= the front internal node's; internal nodes in
//       creation order; a leaf's depth is its length
//   (d) num[d] = leaves per depth, depths above L counted at L; total = sum num[i] << (L - i); while total > 2^L:
//       num[L]--, for the largest i < L with num[i] > 0: num[i]--, num[i + 1] += 2; total--   (at most once per symbol)
//   (e) lengths from num in sorted order: the first num[L] symbols get L, the next num[L - 1] get L - 1, ...
//   (f) canonical codes, RFC 1951 3.2.2
// Loops: the merge n - 1 <= 285 rounds, depths and (e) <= 286, (d) <= 286 rounds of <= 15, codes <= 286.
constexpr int kPngLit = 286, kPngDist = 30, kPngCl = 19;
constexpr int kPngLens = kPngLit + kPngDist;       // the two length lists, the distance list at kPngLit
constexpr uint32_t kPngMaxCount = 1u << 20;
constexpr uint32_t kPngUnusedKey = 0xC0000000u;    // keys of unused symbols sort behind every used one

struct PngCodeScratch {
    uint32_t keys[kPngLit];     // by symbol
    uint32_t sorted[kPngLit];   // ascending, the used ones first
    uint32_t w[kPngLit];        // weights of the internal nodes, then their depths
    uint16_t lp[kPngLit];       // the internal node a leaf hangs on
    uint16_t ip[kPngLit];       // ... an internal node hangs on
};

DP_HD inline uint32_t png_code_key(const uint32_t count, const uint32_t sym)
{
    const uint32_t c = count < kPngMaxCount ? count : kPngMaxCount;
    return c ? (c << 9) | sym : kPngUnusedKey | sym;
}

// rule (a) on the keys (the counts themselves stay what was counted); -> the number of used symbols.  m >= 2.
DP_HD inline int png_pad_keys(uint32_t *keys, const int m)
{
    int used = 0;
    for (int s = 0; s < m; ++s) used += keys[s] < kPngUnusedKey;
    for (int s = 0; s < m && used < 2; ++s)
        if (keys[s] >= kPngUnusedKey) {
            keys[s] = png_code_key(1u, (uint32_t)s);
            ++used;
        }
    return used;
}

// rules (c), (d), (e) on the sorted keys of n >= 2 used symbols out of m; 2^L >= n
DP_HD inline void png_code_lengths_sorted(const uint32_t *sorted, const int n, const int m, const int L, uint8_t *lengths, uint32_t *w,
                                          uint16_t *lp, uint16_t *ip)
{
    for (int s = 0; s < m; ++s) lengths[s] = 0;
    int li = 0, ni = 0;
    for (int k = 0; k < n - 1; ++k) {   // node k is made of the two lightest
        uint32_t sum = 0;
        for (int two = 0; two < 2; ++two) {
            if (li < n && (ni >= k || (sorted[li] >> 9) <= w[ni])) {
                lp[li] = (uint16_t)k;
                sum += sorted[li] >> 9;
                ++li;
            } else {
                ip[ni] = (uint16_t)k;
                sum += w[ni];
                ++ni;
            }
        }
        w[k] = sum;
    }
    w[n - 2] = 0;   // the root; from here on w[] holds depths
    for (int k = n - 3; k >= 0; --k) w[k] = w[ip[k]] + 1u;
    uint32_t num[16];
    for (int d = 0; d < 16; ++d) num[d] = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t d = w[lp[i]] + 1u;
        ++num[d < (uint32_t)L ? d : (uint32_t)L];
    }
    uint32_t total = 0;
    for (int i = 1; i <= L; ++i) total += num[i] << (L - i);
    for (int round = 0; round < n && total > (1u << L); ++round) {
        --num[L];
        for (int i = L - 1; i > 0; --i)
            if (num[i]) {
                --num[i];
                num[i + 1] += 2;
                break;
            }
        --total;
    }
    int at = 0;
    for (int d = L; d > 0; --d)
        for (uint32_t k = 0; k < num[d] && at < n; ++k, ++at) lengths[sorted[at] & 511u] = (uint8_t)d;
}

// rule (f): codes[s] = the code as it enters the stream (first bit lowest) | length << 16
DP_HD inline void png_canonical_codes(const uint8_t *lengths, const int m, uint32_t *codes)
{
    uint32_t count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int s = 0; s < m; ++s) ++count[lengths[s] & 15];
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int s = 0; s < m; ++s) {
        const int nb = lengths[s] & 15;
        codes[s] = nb ? png_rev(next[nb]++, nb) | ((uint32_t)nb << 16) : 0u;
    }
}

// HLIT = max(257, the highest literal/length symbol with a length + 1); HDIST = the highest distance symbol with one + 1
DP_HD inline int png_hlit(const uint8_t *lit)
{
    int n = kPngLit;
    while (n > 257 && lit[n - 1] == 0) --n;
    return n;
}
DP_HD inline int png_hdist(const uint8_t *dist)
{
    int n = kPngDist;
    while (n > 1 && dist[n - 1] == 0) --n;
    return n;
}

DP_HD inline int png_cl_extra(const uint32_t sym) { return sym == 16u ? 2 : sym == 17u ? 3 : sym == 18u ? 7 : 0; }

// The two length lists as one sequence (runs cross the boundary), run-length coded greedily: a run of r zeros at i is symbol
// 18 over min(r, 138) when r >= 11, symbol 17 over r when r >= 3, else one literal 0; a run of a length v is the literal v and,
// while the rest is >= 3, symbol 16 over min(rest, 6) -- a rest of 1 or 2 is met again as a run of its own.
// seq[k] = symbol | extra value << 5; cl_counts[19] receives the histogram; -> the number of entries (<= hlit + hdist).
DP_HD inline int png_cl_sequence(const uint8_t *lit, const int hlit, const uint8_t *dist, const int hdist, uint16_t *seq, uint32_t *cl_counts)
{
    for (int s = 0; s < kPngCl; ++s) cl_counts[s] = 0;
    const int total = hlit + hdist;
    int nseq = 0;
    for (int i = 0; i < total;) {   // <= 316
        const uint32_t v = i < hlit ? lit[i] : dist[i - hlit];
        int r = 1;
        while (i + r < total && (i + r < hlit ? lit[i + r] : dist[i + r - hlit]) == v) ++r;
        uint32_t sym, val = 0;
        int covered;
        if (v == 0 && r >= 11) { covered = r < 138 ? r : 138; sym = 18u; val = (uint32_t)covered - 11u; }
        else if (v == 0 && r >= 3) { covered = r; sym = 17u; val = (uint32_t)r - 3u; }
        else { covered = 1; sym = v; }
        seq[nseq++] = (uint16_t)(sym | (val << 5));
        ++cl_counts[sym];
        i += covered;
        if (v != 0)
            for (int rest = r - 1; rest >= 3;) {
                const int k = rest < 6 ? rest : 6;
                seq[nseq++] = (uint16_t)(16u | ((uint32_t)(k - 3) << 5));
                ++cl_counts[16];
                i += k;
                rest -= k;
            }
    }
    return nseq;
}

DP_HD inline uint32_t png_cl_order(const int i)   // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
{
    return i < 3 ? 16u + (uint32_t)i : i == 3 ? 0u : (i & 1) ? 8u - (uint32_t)((i - 3) / 2) : 8u + (uint32_t)((i - 4) / 2);
}

DP_HD inline int png_hclen(const uint8_t *cl)   // max(4, 1 + the last index of the order whose symbol has a length)
{
    int n = kPngCl;
    while (n > 4 && cl[png_cl_order(n - 1)] == 0) --n;
    return n;
}

// the bits of one entry of the code-length sequence: its code, then its extra bits (<= 7 + 7)
DP_HD inline PngBits png_cl_entry(const uint32_t entry, const uint32_t *cl_codes)
{
    const uint32_t sym = entry & 31u, c = cl_codes[sym];
    PngBits t;
    t.nb = (int)(c >> 16);
    t.bits = (c & 0xFFFFu) | ((entry >> 5) << t.nb);
    t.nb += png_cl_extra(sym);
    return t;
}

// A token as one word (the device's token area holds these): a literal is its byte; a match is bit 31, the length in bits
// 0 ... 8 and the distance - 1 in bits 9 ... 23.
DP_HD inline uint32_t png_token_literal(const uint32_t byte) { return byte; }
DP_HD inline uint32_t png_token_match(const int len, const int dist) { return 0x80000000u | (uint32_t)len | ((uint32_t)(dist - 1) << 9); }

DP_HD inline PngBits png_fixed_token(const uint32_t word)
{
    return (word >> 31) ? png_fixed_match((int)(word & 511u), (int)((word >> 9) & 0x7FFFu) + 1) : png_fixed_literal(word & 255u);
}

struct PngBits64 {
    uint64_t bits;   // LSB first
    int nb;          // <= 15 + 5 + 15 + 13 = 48
};

DP_HD inline PngBits64 png_dynamic_token(const uint32_t word, const uint32_t *lit_codes, const uint32_t *dist_codes)
{
    PngBits64 t;
    if (!(word >> 31)) {
        const uint32_t c = lit_codes[word & 255u];
        t.bits = c & 0xFFFFu;
        t.nb = (int)(c >> 16);
        return t;
    }
    uint32_t sym, lval, dcode, dval;
    int lextra, dextra;
    png_length_code((int)(word & 511u), sym, lextra, lval);
    png_dist_code((int)((word >> 9) & 0x7FFFu) + 1, dcode, dextra, dval);
    const uint32_t lc = lit_codes[sym], dc = dist_codes[dcode];
    t.bits = lc & 0xFFFFu;
    t.nb = (int)(lc >> 16);
    t.bits |= (uint64_t)lval << t.nb;
    t.nb += lextra;
    t.bits |= (uint64_t)(dc & 0xFFFFu) << t.nb;
    t.nb += (int)(dc >> 16);
    t.bits |= (uint64_t)dval << t.nb;
    t.nb += dextra;
    return t;
}

// what a token adds to the histograms (hist[0 .. 286) literal/length, hist[286 .. 316) distance) and to the two bit totals
DP_HD inline void png_token_symbols(const uint32_t word, uint32_t &lit_sym, int &dist_sym, int &extra_bits, int &fixed_bits)
{
    if (!(word >> 31)) {
        lit_sym = word & 255u;
        dist_sym = -1;
        extra_bits = 0;
        fixed_bits = lit_sym < 144u ? 8 : 9;
        return;
    }
    uint32_t lval, dcode, dval;
    int lextra, dextra;
    png_length_code((int)(word & 511u), lit_sym, lextra, lval);
    png_dist_code((int)((word >> 9) & 0x7FFFu) + 1, dcode, dextra, dval);
    dist_sym = (int)dcode;
    extra_bits = lextra + dextra;
    fixed_bits = (lit_sym < 280u ? 7 : 8) + 5 + extra_bits;
}

// rule (a) ... (e) for one alphabet on the host (the device sorts with the wave: png.hip)
inline void png_code_lengths(const uint32_t *counts, const int m, const int L, uint8_t *lengths, PngCodeScratch &sc)
{
    for (int s = 0; s < m; ++s) sc.keys[s] = png_code_key(counts[s], (uint32_t)s);
    const int n = png_pad_keys(sc.keys, m);
    std::copy(sc.keys, sc.keys + m, sc.sorted);
    std::sort(sc.sorted, sc.sorted + m);
    png_code_lengths_sorted(sc.sorted, n, m, L, lengths, sc.w, sc.lp, sc.ip);
}

// Everything a dynamic block's header says, and the block's bits from its three header bits through end-of-block, from the
// histograms (hist[256] == 1), the extra-bit total and the code lengths alone.
struct PngDynPlan {
    uint8_t lens[kPngLens + kPngCl];   // literal/length, distance at kPngLit, code-length alphabet at kPngLens
    uint32_t codes[kPngLens + kPngCl];
    uint16_t seq[kPngLens];
    int hlit, hdist, hclen, nseq;
    uint64_t bits;
};

inline void png_dynamic_plan(const uint32_t *hist, const uint64_t extra_bits, PngDynPlan &p, PngCodeScratch &sc)
{
    uint32_t cl_counts[kPngCl];
    png_code_lengths(hist, kPngLit, 15, p.lens, sc);
    png_code_lengths(hist + kPngLit, kPngDist, 15, p.lens + kPngLit, sc);
    p.hlit = png_hlit(p.lens);
    p.hdist = png_hdist(p.lens + kPngLit);
    p.nseq = png_cl_sequence(p.lens, p.hlit, p.lens + kPngLit, p.hdist, p.seq, cl_counts);
    png_code_lengths(cl_counts, kPngCl, 7, p.lens + kPngLens, sc);
    p.hclen = png_hclen(p.lens + kPngLens);
    p.bits = 3u + 5u + 5u + 4u + 3u * (uint64_t)p.hclen + extra_bits;
    for (int k = 0; k < p.nseq; ++k) p.bits += (uint64_t)p.lens[kPngLens + (p.seq[k] & 31u)] + (uint64_t)png_cl_extra(p.seq[k] & 31u);
    for (int s = 0; s < kPngLens; ++s) p.bits += (uint64_t)hist[s] * p.lens[s];
    png_canonical_codes(p.lens, kPngLit, p.codes);
    png_canonical_codes(p.lens + kPngLit, kPngDist, p.codes + kPngLit);
    png_canonical_codes(p.lens + kPngLens, kPngCl, p.codes + kPngLens);
}

// One plane -> `out` (cleared first): a complete zlib stream.  png_geometry_ok(h, w, depth, seg_bytes) is the caller's.
// dynamic == false: stored and fixed blocks (png_deflate_encode); true: the third candidate as well (png_deflate_encode_dyn).
inline void png_deflate_encode_blocks(const uint8_t *plane, const int h, const int w, const int depth, const int seg_bytes, const bool dynamic,
                                      std::vector<uint8_t> &out)
{
    const uint32_t rb = png_row_bytes(w, depth);
    const int64_t F = png_filtered_size(h, w, depth);
    const int64_t seg = std::min<int64_t>(seg_bytes, F), n_seg = png_segments(F, seg_bytes);
    out.clear();
    out.push_back(0x78);
    out.push_back(0x01);
    std::vector<uint8_t> s((size_t)seg);
    std::vector<uint32_t> cand((size_t)seg), heads((size_t)1 << kPngHashBits), toks;
    std::vector<uint32_t> hist((size_t)kPngLens);
    PngCodeScratch sc;
    PngDynPlan plan;
    toks.reserve((size_t)seg);
    uint32_t A = 1, B = 0;
    for (int64_t j = 0; j < n_seg; ++j) {
        const int64_t at = j * seg;
        const uint32_t n = (uint32_t)std::min<int64_t>(seg, F - at);
        const bool last = j == n_seg - 1;
        uint64_t s1 = 0, s2 = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t o = (uint32_t)(at + i), r = o / rb;
            s[i] = (uint8_t)png_filtered_byte(plane, w, depth, r, o - r * rb);
            s1 += s[i];
            s2 += (uint64_t)(n - i) * s[i];
        }
        B = (uint32_t)((B + (uint64_t)n * A + s2 % kAdlerMod) % kAdlerMod);
        A = (uint32_t)((A + s1) % kAdlerMod);
        // candidates: a function of the bytes alone
        std::fill(heads.begin(), heads.end(), kPngNoCand);
        for (uint32_t p = 0; p + 2 < n; ++p) {
            const uint32_t hsh = png_hash3(s[p], s[p + 1], s[p + 2]);
            cand[p] = heads[hsh];
            heads[hsh] = p;
        }
        toks.clear();
        std::fill(hist.begin(), hist.end(), 0u);
        uint64_t fixed_bits = 3, extra_bits = 0;
        for (uint32_t p = 0; p < n;) {
            uint32_t len = 0, q = kPngNoCand;
            if (p + 2 < n && (q = cand[p]) != kPngNoCand) {
                const uint32_t maxlen = std::min<uint32_t>(258u, n - p);
                while (len < maxlen && s[q + len] == s[p + len]) ++len;
            }
            uint32_t word;
            if (len >= 3) {
                word = png_token_match((int)len, (int)(p - q));
                p += len;
            } else {
                word = png_token_literal(s[p]);
                ++p;
            }
            uint32_t lit_sym;
            int dist_sym, eb, fb;
            png_token_symbols(word, lit_sym, dist_sym, eb, fb);
            ++hist[lit_sym];
            if (dist_sym >= 0) ++hist[(size_t)kPngLit + (size_t)dist_sym];
            extra_bits += (uint64_t)eb;
            fixed_bits += (uint64_t)fb;
            toks.push_back(word);
        }
        fixed_bits += 7;   // end of block: symbol 256
        const uint32_t stored_bytes = png_stored_segment_bytes(n, last), fixed_bytes = png_huffman_segment_bytes(fixed_bits, last);
        int type = png_segment_choice(stored_bytes, fixed_bytes);
        if (dynamic) {
            hist[256] = 1;
            png_dynamic_plan(hist.data(), extra_bits, plan, sc);
            type = png_segment_choice(stored_bytes, fixed_bytes, png_huffman_segment_bytes(plan.bits, last));
        }
        if (type == kPngStored) {
            out.push_back(last ? 1 : 0);
            out.push_back((uint8_t)(n & 0xFFu));
            out.push_back((uint8_t)(n >> 8));
            out.push_back((uint8_t)(~n & 0xFFu));
            out.push_back((uint8_t)((~n >> 8) & 0xFFu));
            out.insert(out.end(), s.begin(), s.begin() + (std::ptrdiff_t)n);
            if (!last) out.insert(out.end(), {0x00, 0x00, 0x00, 0xFF, 0xFF});
            continue;
        }
        GifBits bits;   // (an LSB-first bit writer)
        bits.put((last ? 1u : 0u) | ((uint32_t)type << 1), 3);
        if (type == kPngFixed) {
            for (const uint32_t word : toks) {
                const PngBits t = png_fixed_token(word);
                bits.put(t.bits, t.nb);
            }
            bits.put(0, 7);
        } else {
            bits.put((uint32_t)(plan.hlit - 257) | ((uint32_t)(plan.hdist - 1) << 5) | ((uint32_t)(plan.hclen - 4) << 10), 14);
            for (int i = 0; i < plan.hclen; ++i) bits.put(plan.lens[kPngLens + png_cl_order(i)], 3);
            for (int k = 0; k < plan.nseq; ++k) {
                const PngBits t = png_cl_entry(plan.seq[k], plan.codes + kPngLens);
                bits.put(t.bits, t.nb);
            }
            for (const uint32_t word : toks) {
                const PngBits64 t = png_dynamic_token(word, plan.codes, plan.codes + kPngLit);
                bits.put((uint32_t)(t.bits & 0xFFFFFFu), t.nb < 24 ? t.nb : 24);
                if (t.nb > 24) bits.put((uint32_t)(t.bits >> 24), t.nb - 24);
            }
            bits.put(plan.codes[256] & 0xFFFFu, (int)(plan.codes[256] >> 16));
        }
        if (!last) {
            bits.put(0, 3);
            bits.flush();
            for (const uint8_t b : {0x00, 0x00, 0xFF, 0xFF}) bits.data.push_back(b);
        } else {
            bits.flush();
        }
        out.insert(out.end(), bits.data.begin(), bits.data.end());
    }
    const uint32_t adler = (B << 16) | A;
    for (int k = 3; k >= 0; --k) out.push_back((uint8_t)(adler >> (8 * k)));
}

inline void png_deflate_encode(const uint8_t *plane, const int h, const int w, const int depth, const int seg_bytes, std::vector<uint8_t> &out)
{
    png_deflate_encode_blocks(plane, h, w, depth, seg_bytes, false, out);
}

inline void png_deflate_encode_dyn(const uint8_t *plane, const int h, const int w, const int depth, const int seg_bytes, std::vector<uint8_t> &out)
{
    png_deflate_encode_blocks(plane, h, w, depth, seg_bytes, true, out);
}

// ---- PNG chunk CRCs and finished chunks (png_file.hip, include/ditherpie_hip_png_file.h) -----------------------------------
// CRC-32/ISO-HDLC: reflected polynomial 0xEDB88320, register initialised to 0xFFFFFFFF, result inverted.  Everything is a
// polynomial over GF(2) modulo P in the reflected representation: bit 31 of a word is the coefficient of x^0.
//   register   crc32_update(state, bytes): the register after the bytes; crc = ~crc32_update(~0, bytes)
//   pure       the register run from 0 with no inversion: pure(M) = M(x) x^32 mod P.  Linear, and blind to leading zeros:
//              pure(A || B) = pure(A) x^(8 len B) + pure(B).  What the device computes per piece and joins.
//   finish     crc(prefix || M) = ~(state(prefix) x^(8 len M) + pure(M)): the register after the prefix, shifted past M.
// The device cuts a run into pieces of kCrcPieceBytes that END on the last 4-byte boundary of the run's addresses (the up
// to three bytes behind it are fed bit by bit at the end); kCrcPieces of them are what one workgroup covers in one step
// (kCrcSpanBytes).  The bytes in front of the run that the first piece and the first span lack count as zeros.
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr int kCrcPieceBytes = 64;                               // DP_PNG_CRC_PIECE_BYTES
constexpr int kCrcPieces = 256;                                  // one lane each
constexpr int kCrcSpanBytes = kCrcPieceBytes * kCrcPieces;       // DP_PNG_CRC_SPAN_BYTES
constexpr int kPngFileMaxPre = 4096, kPngFileMaxPost = 64;
constexpr int64_t kPngFileMaxStream = (1LL << 31) - 16;          // a stream bound must stay below it

// a b mod P; x^0 is 0x80000000.  Always 32 rounds: the same instruction stream in every lane.
DP_HD constexpr uint32_t crc_gfmul(const uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

DP_HD constexpr uint32_t crc_bits8(uint32_t c)   // eight rounds of the register: c x^8 mod P
{
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
    return c;
}

struct CrcTables {
    uint32_t byte[4][256];        // slicing by four: byte[k][v] is the register after byte v and k zero bytes
    uint32_t piece[kCrcPieces];   // x^(8 kCrcPieceBytes j): what lifts the piece j pieces before the span's last one
    uint32_t x8[32];              // x^(8 2^k): the squares a shift by any byte count below 2^32 is put together from
};

constexpr CrcTables make_crc_tables()
{
    CrcTables t{};
    for (uint32_t v = 0; v < 256; ++v) t.byte[0][v] = crc_bits8(v);
    for (int k = 1; k < 4; ++k)
        for (uint32_t v = 0; v < 256; ++v) t.byte[k][v] = (t.byte[k - 1][v] >> 8) ^ t.byte[0][t.byte[k - 1][v] & 255u];
    t.x8[0] = 0x80000000u >> 8;
    for (int k = 1; k < 32; ++k) t.x8[k] = crc_gfmul(t.x8[k - 1], t.x8[k - 1]);
    uint32_t step = 0x80000000u;                                  // x^(8 kCrcPieceBytes)
    for (int k = 0; k < 32; ++k)
        if ((kCrcPieceBytes >> k) & 1) step = crc_gfmul(step, t.x8[k]);
    t.piece[0] = 0x80000000u;
    for (int j = 1; j < kCrcPieces; ++j) t.piece[j] = crc_gfmul(t.piece[j - 1], step);
    return t;
}
constexpr CrcTables kCrcTables = make_crc_tables();
static_assert(kCrcTables.byte[0][1] == 0x77073096u && kCrcTables.byte[0][255] == 0x2D02EF8Du, "the CRC-32 byte table");
static_assert(kCrcTables.byte[1][1] == crc_bits8(kCrcTables.byte[0][1]), "slicing tables: one more zero byte each");
static_assert(kCrcTables.piece[1] == kCrcTables.x8[6] && kCrcTables.piece[2] == kCrcTables.x8[7] && kCrcSpanBytes == 1 << 14, "64-byte pieces, 16 KiB spans");

// c x^(8 n_bytes) mod P from a table of squares x8 (host: kCrcTables.x8)
DP_HD inline uint32_t crc_shift_bytes(uint32_t c, uint64_t n_bytes, const uint32_t *x8)
{
    for (int k = 0; n_bytes && k < 32; ++k, n_bytes >>= 1)
        if (n_bytes & 1u) c = crc_gfmul(c, x8[k]);
    return c;
}

inline uint32_t crc32_update(uint32_t state, const uint8_t *p, const size_t n)
{
    for (size_t i = 0; i < n; ++i) state = (state >> 8) ^ kCrcTables.byte[0][(state ^ p[i]) & 255u];
    return state;
}
inline uint32_t crc32_bytes(const uint8_t *p, const size_t n) { return ~crc32_update(0xFFFFFFFFu, p, n); }
// the CRC of A || B from the CRCs of A and B: the initial value and the inversion cancel
inline uint32_t crc32_combine(const uint32_t crc_a, const uint32_t crc_b, const uint64_t len_b) { return crc_shift_bytes(crc_a, len_b, kCrcTables.x8) ^ crc_b; }

// Finished chunks.  Frame f of a call: pre_bytes bytes of the caller's, one chunk -- IDAT for f < n_idat, else fdAT with the
// sequence number seq0 + (f - n_idat) seq_step in front of the stream --, post_bytes bytes of the caller's.
DP_HD inline int64_t png_file_clamp(const int64_t size, const int64_t stride) { return size < 0 ? 0 : size > stride ? stride : size; }
DP_HD inline uint32_t png_file_type(const bool fdat) { return fdat ? 0x66644154u : 0x49444154u; }   // big-endian "fdAT", "IDAT"
inline bool png_file_geometry_ok(const int64_t stream_stride, const int pre_bytes, const int post_bytes)
{
    return stream_stride >= 0 && stream_stride < kPngFileMaxStream && pre_bytes >= 0 && pre_bytes <= kPngFileMaxPre && post_bytes >= 0 && post_bytes <= kPngFileMaxPost;
}
inline uint64_t png_file_bound(const int64_t stream_stride, const int pre_bytes, const int post_bytes) { return (uint64_t)pre_bytes + 16u + (uint64_t)stream_stride + (uint64_t)post_bytes; }
inline void png_file_be32(uint8_t *p, const uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// -> the bytes written; offsets[0 ... n_frames] are filled.  `out` holds n_frames * png_file_bound(...) bytes.
inline int64_t png_file_assemble(const uint8_t *streams, const int64_t stream_stride, const int64_t *sizes, const int n_frames, const int n_idat,
                                 const uint32_t seq0, const uint32_t seq_step, const uint8_t *pre, const int64_t pre_stride, const int pre_bytes,
                                 const uint8_t *post, const int post_bytes, uint8_t *out, int64_t *offsets)
{
    int64_t at = 0;
    offsets[0] = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int64_t n = png_file_clamp(sizes[f], stream_stride);
        const bool fdat = f >= n_idat;
        if (pre_bytes) std::memcpy(out + at, pre + (size_t)f * (size_t)pre_stride, (size_t)pre_bytes);
        at += pre_bytes;
        uint8_t *head = out + at;
        png_file_be32(head, (uint32_t)n + (fdat ? 4u : 0u));
        png_file_be32(head + 4, png_file_type(fdat));
        int hdr = 8;
        if (fdat) {
            png_file_be32(head + 8, seq0 + (uint32_t)(f - n_idat) * seq_step);
            hdr = 12;
        }
        if (n) std::memcpy(head + hdr, streams + (size_t)f * (size_t)stream_stride, (size_t)n);
        const uint32_t crc = ~crc32_update(crc32_update(0xFFFFFFFFu, head + 4, (size_t)hdr - 4), head + hdr, (size_t)n);
        png_file_be32(head + hdr + n, crc);
        at += hdr + n + 4;
        if (post_bytes) std::memcpy(out + at, post, (size_t)post_bytes);
        at += post_bytes;
        offsets[f + 1] = at;
    }
    return at;
}

// ---- Dot diffusion: class matrices and their level schedule (dotdiff.hip, include/ditherpie_hip_dotdiff.h) -----------------
//
// A class matrix is m x m (m = 2, 4, 8, 16), a permutation of 0 .. m*m-1, tiled over the plane.  level(cell) is the largest
// number of king moves of a path through the tiled matrix that ends in the cell and along which the class strictly
// increases; reach = the largest level.  Cells of one level are never neighbours (of two neighbours the one of the higher
// class has the higher level) and a cell's level exceeds that of every neighbour of a lower class: the pixels of one level
// can be quantised together once the levels below are done, which is how the kernel walks a tile.
constexpr int kDotDiffMaxReach = 16;        // DP_DOTDIFF_MAX_REACH: the halo a tile of the kernel carries on each side
constexpr int kDotDiffMaxCells = 256;

inline bool dotdiff_matrix_ok(const uint8_t *cls, const int m)
{
    if (!cls || (m != 2 && m != 4 && m != 8 && m != 16)) return false;
    bool seen[kDotDiffMaxCells] = {};
    for (int i = 0; i < m * m; ++i) {
        if ((int)cls[i] >= m * m || seen[cls[i]]) return false;   // (m = 16: every byte is below 256, repeats remain)
        seen[cls[i]] = true;
    }
    return true;
}

// level[cell] for a matrix that dotdiff_matrix_ok accepts (int: a 16 x 16 matrix can reach 255); -> reach
inline int dotdiff_levels(const uint8_t *cls, const int m, int *level)
{
    int cell_of[kDotDiffMaxCells];
    for (int i = 0; i < m * m; ++i) cell_of[cls[i]] = i;
    int reach = 0;
    for (int c = 0; c < m * m; ++c) {       // in class order: every neighbour of a lower class has its level already
        const int cell = cell_of[c], y = cell / m, x = cell % m;
        int lv = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dy && !dx) continue;
                const int n = ((y + dy + m) % m) * m + (x + dx + m) % m;
                if ((int)cls[n] < c) lv = std::max(lv, level[n] + 1);
            }
        level[cell] = lv;
        reach = std::max(reach, lv);
    }
    return reach;
}

// What the kernel is given besides the matrix: the cells ordered by level (ascending, by cell number inside a level) and
// where each level starts in that order.  For a matrix of reach <= kDotDiffMaxReach.
struct DotDiffSchedule {
    uint8_t order[kDotDiffMaxCells];
    uint16_t start[kDotDiffMaxReach + 2];   // level l: order[start[l] .. start[l + 1])
    int n_levels;                           // reach + 1
};

inline void dotdiff_schedule(const int *level, const int m, const int reach, DotDiffSchedule &s)
{
    s.n_levels = reach + 1;
    int at = 0;
    for (int l = 0; l <= reach; ++l) {
        s.start[l] = (uint16_t)at;
        for (int i = 0; i < m * m; ++i)
            if (level[i] == l) s.order[at++] = (uint8_t)i;
    }
    for (int l = reach + 1; l < kDotDiffMaxReach + 2; ++l) s.start[l] = (uint16_t)at;
    for (int i = at; i < kDotDiffMaxCells; ++i) s.order[i] = 0;
}

// ---- Integer error diffusion: the taps of a scan (idiff.hip, include/ditherpie_hip_idiff.h) --------------------------------
//
// A tap (dx, dy, weight) hands weight / divisor of a pixel's error to the pixel dx to the right and dy below.  The kernel
// works with q = floor(weight * strength256 * 256 / divisor), the share in 1/65536, and walks a band of rows on an
// anti-diagonal: the row below trails by `skew` columns, the smallest s >= 1 with s * dy + dx >= 1 for every tap of a later
// row, so that every source of a pixel is finished at least one step before the pixel.
constexpr int kIdiffMaxTaps = 12;

struct IdiffPlan {
    int n, skew;
    int dx[kIdiffMaxTaps], dy[kIdiffMaxTaps];
    uint32_t q[kIdiffMaxTaps];   // sum <= 65536
};

// 0, or which rule of the header the arguments break: 1 a NULL array, 2 n_taps outside 1 .. 12, 3 divisor < 1, 4 strength256
// outside 0 .. 256, 5 a tap outside dy 0 .. 2, dx -2 .. 2, dy == 0 => dx >= 1, 6 a (dx, dy) twice, 7 a negative weight,
// 8 weights that sum to more than the divisor.  The plan is complete only with 0.
inline int idiff_plan(const int32_t *dx, const int32_t *dy, const int32_t *weight, const int n_taps, const int divisor, const int strength256,
                      IdiffPlan &p)
{
    p = IdiffPlan{};
    if (n_taps < 1 || n_taps > kIdiffMaxTaps) return 2;
    if (!dx || !dy || !weight) return 1;
    if (divisor < 1) return 3;
    if (strength256 < 0 || strength256 > 256) return 4;
    int64_t sum = 0;
    bool seen[3][5] = {};
    for (int k = 0; k < n_taps; ++k) {
        if (dy[k] < 0 || dy[k] > 2 || dx[k] < -2 || dx[k] > 2 || (dy[k] == 0 && dx[k] < 1)) return 5;
        if (seen[dy[k]][dx[k] + 2]) return 6;
        seen[dy[k]][dx[k] + 2] = true;
        if (weight[k] < 0) return 7;
        sum += weight[k];
    }
    if (sum > divisor) return 8;
    p.n = n_taps;
    p.skew = 1;
    for (int k = 0; k < n_taps; ++k) {
        p.dx[k] = dx[k];
        p.dy[k] = dy[k];
        p.q[k] = (uint32_t)((int64_t)weight[k] * strength256 * 256 / divisor);   // weight <= divisor: at most 65536
        while (dy[k] >= 1 && p.skew * dy[k] + dx[k] < 1) ++p.skew;                // (at most 3: dx >= -2)
    }
    return 0;
}

// ---- Cell-palette dithering: the candidates of a cell and the perturbation (cells.hip, include/ditherpie_hip_cells.h) ------
//
// Every cell may show `colours` = k entries of its choice besides the entries of `fixed`.  The candidates are enumerated
// group by group in the order given; within a group the sets T are the k-subsets of the group's entries outside `fixed`, in
// lexicographic order of their ascending index tuples, and the candidate is S = T | fixed.  At most 4 C(16, 4) = 7280.
// The enumeration is stated once: cells_plan validates and counts, cells_unrank maps a rank to its mask (host and device).
constexpr int kCellPalMaxK = 16, kCellPalMaxColours = 4, kCellPalMaxGroups = 4, kCellPalMaxCandidates = 7280;

DP_HD inline uint32_t cells_binom(const int n, const int k)   // C(n, k) for n <= 16, k <= 4; 0 for k > n or k < 0
{
    if (k < 0 || k > n) return 0u;
    uint32_t c = 1u;
    for (int i = 1; i <= k; ++i) c = c * (uint32_t)(n - k + i) / (uint32_t)i;   // C(n-k+i, i): exact at every step
    return c;
}

DP_HD inline int cells_popcount16(uint32_t v)
{
    int n = 0;
    for (v &= 0xffffu; v; v &= v - 1u) ++n;
    return n;
}

struct CellsPlan {
    uint16_t avail[kCellPalMaxGroups];       // group & ~fixed: what a candidate of the group chooses from
    uint16_t first[kCellPalMaxGroups + 1];   // the rank of the group's first candidate; first[n_groups] = the count
    uint16_t fixed;
    int colours, n_groups;
};

// -> the number of candidates, or -1: K outside 1 .. 16, colours outside 1 .. 4, n_groups outside 1 .. 4, no groups, a bit of
// fixed or of a group at or above K, an empty group, a group with fewer than `colours` entries outside fixed
inline int cells_plan(const int K, const int colours, const uint32_t fixed, const uint16_t *groups, const int n_groups, CellsPlan &p)
{
    if (K < 1 || K > kCellPalMaxK || colours < 1 || colours > kCellPalMaxColours || n_groups < 1 || n_groups > kCellPalMaxGroups || !groups)
        return -1;
    const uint32_t beyond = ~((1u << K) - 1u);
    if (fixed & beyond) return -1;
    p = CellsPlan{};
    p.fixed = (uint16_t)fixed;
    p.colours = colours;
    p.n_groups = n_groups;
    uint32_t at = 0;
    for (int g = 0; g < n_groups; ++g) {
        const uint32_t grp = groups[g];
        if (!grp || (grp & beyond)) return -1;
        p.avail[g] = (uint16_t)(grp & ~fixed);
        const int n = cells_popcount16(p.avail[g]);
        if (n < colours) return -1;
        p.first[g] = (uint16_t)at;
        at += cells_binom(n, colours);
    }
    for (int g = n_groups; g <= kCellPalMaxGroups; ++g) p.first[g] = (uint16_t)at;
    return (int)at;
}

// the mask S of candidate `rank` (rank < first[n_groups])
DP_HD inline uint32_t cells_unrank(const CellsPlan &p, const uint32_t rank)
{
    int g = 0;
    while (g + 1 < p.n_groups && rank >= p.first[g + 1]) ++g;
    uint32_t r = rank - p.first[g], left = p.avail[g], mask = 0u;
    int n = cells_popcount16(left), k = p.colours;
    for (int j = 0; j < kCellPalMaxK && k > 0; ++j) {
        if (!((left >> j) & 1u)) continue;
        --n;                                           // entries of the group above j
        const uint32_t with = cells_binom(n, k - 1);   // candidates whose next entry is j
        if (r < with) {
            mask |= 1u << j;
            --k;
        } else {
            r -= with;
        }
    }
    return mask | p.fixed;
}

// B_m[y mod m][x mod m], the Bayer rank matrix of pattern dithering: B_2 = [[0, 2], [3, 1]], B_2m = 4 B_m(low bits) + B_2(top bit)
inline int cells_bayer_rank(const int m, const int y, const int x)
{
    const int bits = m == 8 ? 3 : (m == 4 ? 2 : 1);
    int r = 0;
    for (int j = 0; j < bits; ++j) {
        const int yb = (y >> j) & 1, xb = (x >> j) & 1;
        r |= (((xb ^ yb) << 1) | yb) << (2 * (bits - 1 - j));
    }
    return r;
}

// t[y * m + x] = floor(((2 B_m[y][x] + 1 - m^2) * spread) / (2 m^2)) for m in {2, 4, 8}, spread 0 .. 255: -128 .. 127
inline void cells_perturbation(const int m, const int spread, int8_t *t)
{
    const int mm = m * m;
    for (int y = 0; y < m; ++y)
        for (int x = 0; x < m; ++x) {
            const int v = (2 * cells_bayer_rank(m, y, x) + 1 - mm) * spread;
            const int d = 2 * mm;
            t[y * m + x] = (int8_t)(v >= 0 ? v / d : -((-v + d - 1) / d));
        }
}

// ---- Void-and-cluster rank matrices (voidcluster.hip, include/ditherpie_hip_voidcluster.h) ---------------------------------
//
// Ulichney's generator on a torus in integer arithmetic: the energy of a cell is the sum of W[squared minimum-image distance]
// over the set cells, W a Gaussian in units of 2^-20 that is zero beyond d2 = D.  What decides a value is a DP_HD function,
// run by this statement and by the kernel alike; the kernel replaces only the schedule.
constexpr int kVacMinSize = 8, kVacMaxSize = 128, kVacMinSigma256 = 256, kVacMaxSigma256 = 768;
constexpr int kVacMaxWeights = 263;   // D + 1 at sigma256 = 768

struct VacWeights {
    int32_t w[kVacMaxWeights];   // w[d2], 0 beyond D
    int D;                       // the last squared distance of a non-zero weight
};

inline bool vac_args_ok(const int h, const int w, const int sigma256)
{
    return h >= kVacMinSize && h <= kVacMaxSize && w >= kVacMinSize && w <= kVacMaxSize && sigma256 >= kVacMinSigma256 &&
           sigma256 <= kVacMaxSigma256;
}

inline void vac_weights(const int sigma256, VacWeights &W)
{
    W.D = -1;
    for (int d2 = 0; d2 < kVacMaxWeights; ++d2) {
        const double v = std::floor(std::exp(-((double)d2 * 32768.0) / ((double)sigma256 * (double)sigma256)) * 1048576.0 + 0.5);
        W.w[d2] = (int32_t)v;
        if (W.w[d2] > 0) W.D = d2;   // (the weights fall monotonically: nothing follows the first zero)
    }
}

DP_HD inline uint32_t vac_mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The seed order of cell i.  mix32 is a bijection of uint32, so the keys of distinct cells differ: (key, i) orders like key.
DP_HD inline uint32_t vac_key(const uint32_t i, const uint32_t seed) { return vac_mix32(vac_mix32(i) ^ seed); }

// a^2 + b^2 of the minimum image between (y, x) and (qy, qx)
DP_HD inline int vac_d2(const int y, const int x, const int qy, const int qx, const int h, const int w)
{
    int a = y > qy ? y - qy : qy - y, b = x > qx ? x - qx : qx - x;
    a = a < h - a ? a : h - a;
    b = b < w - b ? b : w - b;
    return a * a + b * b;
}

// ranks[h * w]; *rounds (may be null) receives the number of relaxation rounds
inline void vac_generate(const int h, const int w, const uint32_t seed, const int sigma256, uint16_t *ranks, int *rounds)
{
    const int n = h * w;
    VacWeights W;
    vac_weights(sigma256, W);
    int R = 0;
    while ((R + 1) * (R + 1) <= W.D) ++R;
    std::vector<int32_t> E((size_t)n, 0);
    std::vector<uint8_t> on((size_t)n, 0), proto;
    // the rows and columns a flip at (qy, qx) reaches, each once: the window where it is narrower than the matrix, else all
    const auto flip = [&](const int q, const int sign) {
        const int qy = q / w, qx = q - qy * w;
        const int ny = 2 * R + 1 < h ? 2 * R + 1 : h, nx = 2 * R + 1 < w ? 2 * R + 1 : w;
        for (int i = 0; i < ny; ++i) {
            const int y = ny < h ? (qy - R + i + h) % h : i;
            for (int j = 0; j < nx; ++j) {
                const int x = nx < w ? (qx - R + j + w) % w : j;
                const int d2 = vac_d2(y, x, qy, qx, h, w);
                if (d2 <= W.D) E[(size_t)y * w + x] += sign * W.w[d2];
            }
        }
        on[q] = sign > 0;
    };
    const auto tightest = [&]() {   // the set cell of the largest energy, the lowest index on ties
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (on[i] && (best < 0 || E[i] > E[best])) best = i;
        return best;
    };
    const auto emptiest = [&]() {   // the unset cell of the smallest energy, the lowest index on ties
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (!on[i] && (best < 0 || E[i] < E[best])) best = i;
        return best;
    };
    const int n1 = std::max(1, n / 10);
    std::vector<uint32_t> keys((size_t)n);
    for (int i = 0; i < n; ++i) keys[i] = vac_key((uint32_t)i, seed);
    std::vector<uint32_t> sorted(keys);
    std::nth_element(sorted.begin(), sorted.begin() + (n1 - 1), sorted.end());
    const uint32_t last = sorted[n1 - 1];
    for (int i = 0; i < n; ++i)
        if (keys[i] <= last) flip(i, +1);
    int r = 0;
    for (bool done = false; r < 4 * n && !done; ++r) {
        const int c = tightest();
        flip(c, -1);
        const int v = emptiest();
        flip(v, +1);
        done = v == c;
    }
    if (rounds) *rounds = r;
    proto = on;
    for (int k = n1 - 1; k >= 0; --k) {
        const int c = tightest();
        flip(c, -1);
        ranks[c] = (uint16_t)k;
    }
    for (int i = 0; i < n; ++i)   // the energy is zero again: integer weights
        if (proto[i]) flip(i, +1);
    for (int k = n1; k < n; ++k) {
        const int v = emptiest();
        flip(v, +1);
        ranks[v] = (uint16_t)k;
    }
}

// thr[i] = float32((2 floor(rank L / n) + 1) / (2 L)), L = min(n, 4096)
inline void vac_thresholds(const uint16_t *ranks, const int n, float *thr)
{
    const int L = std::min(n, 4096);
    for (int i = 0; i < n; ++i) thr[i] = (float)((double)(2 * ((int)ranks[i] * L / n) + 1) / (double)(2 * L));
}

// ---- the Oklab colour metric (include/ditherpie_hip_metric.h; tests/metric_ref.py states it in numpy) -------------------------------
// All integer arithmetic.  LIN[v] = round(65535 f(v / 255)), f the sRGB decoding function: the literal (one for the host and,
// through metric.hip's __constant__ copy, the device); tests/test_metric_cpu.py checks it against the formula.
#define DP_METRIC_LIN_VALUES \
    0, 20, 40, 60, 80, 99, 119, 139, 159, 179, 199, 219, 241, 264, 288, 313, \
    340, 367, 396, 427, 458, 491, 526, 562, 599, 637, 677, 718, 761, 805, 851, 898, \
    947, 997, 1048, 1101, 1156, 1212, 1270, 1330, 1391, 1453, 1517, 1583, 1651, 1720, 1790, 1863, \
    1937, 2013, 2090, 2170, 2250, 2333, 2418, 2504, 2592, 2681, 2773, 2866, 2961, 3058, 3157, 3258, \
    3360, 3464, 3570, 3678, 3788, 3900, 4014, 4129, 4247, 4366, 4488, 4611, 4736, 4864, 4993, 5124, \
    5257, 5392, 5530, 5669, 5810, 5953, 6099, 6246, 6395, 6547, 6700, 6856, 7014, 7174, 7335, 7500, \
    7666, 7834, 8004, 8177, 8352, 8528, 8708, 8889, 9072, 9258, 9445, 9635, 9828, 10022, 10219, 10417, \
    10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909, \
    14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001, \
    18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721, \
    23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094, \
    28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143, \
    34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891, \
    41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359, \
    48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567, \
    57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535
static const uint16_t kMetricLin[256] = {DP_METRIC_LIN_VALUES};
static const uint32_t kMetricA[3][3] = {{27015, 35149, 3372}, {13887, 44611, 7038}, {5787, 18463, 41286}};   // rows sum to 65536
static const int32_t kMetricB[3][3] = {{862, 3251, -17}, {8102, -9948, 1846}, {106, 3206, -3312}};           // rows sum to 4096, 0, 0

// floor(cbrt(x * 2^32)), x < 2^16: the largest c in 0 .. 65535 with c^3 <= x << 32, by bisection
inline uint32_t metric_icbrt(const uint32_t x)
{
    const uint64_t big = (uint64_t)x << 32;
    uint32_t c = 0;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) {
        const uint64_t t = c | bit;
        if (t * t * t <= big) c |= bit;
    }
    return c;
}

// the 65536 values of metric_icbrt, computed once
inline const uint16_t *metric_cbrt_table()
{
    static const std::vector<uint16_t> tab = [] {
        std::vector<uint16_t> t(65536);
        for (uint32_t x = 0; x < 65536; ++x) t[x] = (uint16_t)metric_icbrt(x);
        return t;
    }();
    return tab.data();
}

// (L, a, b) of an sRGB colour; cbrt_tab = metric_cbrt_table() (or nullptr: bisection per component)
inline void metric_lab(const uint32_t r, const uint32_t g, const uint32_t b, const uint16_t *cbrt_tab, int32_t lab[3])
{
    const uint32_t lin[3] = {kMetricLin[r & 255u], kMetricLin[g & 255u], kMetricLin[b & 255u]};
    int32_t c[3];
    for (int i = 0; i < 3; ++i) {
        const uint32_t x = (kMetricA[i][0] * lin[0] + kMetricA[i][1] * lin[1] + kMetricA[i][2] * lin[2]) >> 16;   // < 2^32 before the shift
        c[i] = (int32_t)(cbrt_tab ? cbrt_tab[x] : metric_icbrt(x));
    }
    for (int i = 0; i < 3; ++i) {
        const int32_t v = kMetricB[i][0] * c[0] + kMetricB[i][1] * c[1] + kMetricB[i][2] * c[2];
        lab[i] = v >= 0 ? v >> 14 : -((-v + 16383) >> 14);   // floor, spelled without a shift of a negative value
    }
}

// K <= 256 and every value an integer in [0, 255]: what the metric's table and dp_metric_top2_host take
inline bool metric_palette_ok(const float *pal_f32, const int K)
{
    if (K < 1 || K > 256) return false;
    for (int i = 0; i < 3 * K; ++i)
        if (!(pal_f32[i] >= 0.0f && pal_f32[i] <= 255.0f && pal_f32[i] == std::floor(pal_f32[i]))) return false;
    return true;
}

// coordinates of the palette under the metric: K x 3 (metric 0: the bytes themselves)
inline void metric_palette_coords(const float *pal_f32, const int K, const int oklab, int32_t *coords)
{
    const uint16_t *ct = oklab ? metric_cbrt_table() : nullptr;
    for (int k = 0; k < K; ++k) {
        const uint32_t r = (uint32_t)pal_f32[3 * k], g = (uint32_t)pal_f32[3 * k + 1], b = (uint32_t)pal_f32[3 * k + 2];
        if (oklab) metric_lab(r, g, b, ct, coords + 3 * k);
        else coords[3 * k] = (int32_t)r, coords[3 * k + 1] = (int32_t)g, coords[3 * k + 2] = (int32_t)b;
    }
}

// The two smallest (d(q, k), k) of n colours, compared as pairs: the lowest index wins on equal distance; K = 1: both 0.
// d0 / d1 (may be null) receive the two distances.
inline void metric_top2(const uint8_t *rgb, const int64_t n, const int32_t *coords, const int K, const int oklab, uint8_t *idx0, uint8_t *idx1,
                        int32_t *d0_out, int32_t *d1_out)
{
    const uint16_t *ct = oklab ? metric_cbrt_table() : nullptr;
    for (int64_t i = 0; i < n; ++i) {
        int32_t q[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        if (oklab) metric_lab(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], ct, q);
        int32_t d0 = std::numeric_limits<int32_t>::max(), d1 = d0;
        int i0 = 0, i1 = 0;
        for (int k = 0; k < K; ++k) {   // ascending k and strict comparisons: an equal distance never displaces a lower index
            const int32_t x = q[0] - coords[3 * k], y = q[1] - coords[3 * k + 1], z = q[2] - coords[3 * k + 2];
            const int32_t d = x * x + y * y + z * z;   // <= 408 098 306
            if (d < d0) {
                d1 = d0, i1 = i0;
                d0 = d, i0 = k;
            } else if (d < d1) {
                d1 = d, i1 = k;
            }
        }
        if (K == 1) d1 = d0, i1 = 0;
        idx0[i] = (uint8_t)i0;
        idx1[i] = (uint8_t)i1;
        if (d0_out) d0_out[i] = d0;
        if (d1_out) d1_out[i] = d1;
    }
}

// the ordered decision: nearest iff d0 / (d0 + d1) <= t in IEEE float64, the quotient 0 when the sum is 0
inline bool metric_takes_nearest(const int32_t d0, const int32_t d1, const float t)
{
    const double s = (double)d0 + (double)d1;
    const double f = s > 0.0 ? (double)d0 / s : 0.0;
    return f <= (double)t;
}

// ---- Oklab palette fitting (include/ditherpie_hip_okfit.h; tests/okfit_ref.py states it in numpy) ----------------------------------
// The host statement of the fit: greedy k-means++ seeding, Lloyd passes with rounded integer means, the medoid of every centre.
// Integers throughout; ascending loops with strict comparisons give the tie rules (the lowest code, the lowest centre index).
constexpr int kOkfitMaxK = 256;
constexpr int kOkfitMaxIter = 10000;
constexpr int64_t kOkfitMaxPoints = (int64_t)1 << 24;

// 0, or which rule the arguments break: 1 a size (n, K < 1, max_iter), 2 K above 256, 3 the codes, 4 the counts
inline int okfit_check(const uint32_t *codes, const uint32_t *counts, const int64_t n, const int K, const int max_iter)
{
    if (n < 1 || n > kOkfitMaxPoints || K < 1 || max_iter < 1 || max_iter > kOkfitMaxIter) return 1;
    if (K > kOkfitMaxK) return 2;
    uint64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (codes[i] >= (1u << 24) || (i > 0 && codes[i] <= codes[i - 1])) return 3;
        if (counts[i] == 0) return 4;
        total += counts[i];
    }
    return total >= ((uint64_t)1 << 32) ? 4 : 0;
}

inline int64_t okfit_dist(const int32_t *p, const int32_t *c)
{
    const int64_t x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
    return x * x + y * y + z * z;
}

// floor(a / b), b > 0
inline int64_t okfit_floordiv(const int64_t a, const int64_t b)
{
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// labels[i] = the centre of least distance (the lowest index on ties), dist[i] that distance
inline void okfit_assign(const int32_t *P, const int64_t n, const int32_t *C, const int K, int32_t *labels, int64_t *dist)
{
    for (int64_t i = 0; i < n; ++i) {
        int64_t best = okfit_dist(P + 3 * i, C);
        int32_t at = 0;
        for (int k = 1; k < K; ++k) {
            const int64_t d = okfit_dist(P + 3 * i, C + 3 * k);
            if (d < best) best = d, at = k;
        }
        labels[i] = at;
        dist[i] = best;
    }
}

// palette K x 3 bytes, centres K x 3; the arguments have passed okfit_check
inline void okfit_host(const uint32_t *codes, const uint32_t *counts, const int64_t n, const int K, const int max_iter, uint8_t *palette,
                       int32_t *centres, int *n_iter_out, uint64_t *distortion_out)
{
    const uint16_t *ct = metric_cbrt_table();
    std::vector<int32_t> P((size_t)3 * n), C((size_t)3 * K), labels((size_t)n);
    std::vector<int64_t> dist((size_t)n), S((size_t)3 * K);
    std::vector<uint64_t> cnt((size_t)K);
    for (int64_t i = 0; i < n; ++i) metric_lab(codes[i] >> 16, (codes[i] >> 8) & 255u, codes[i] & 255u, ct, &P[3 * (size_t)i]);
    // seeding
    int64_t first = 0;
    for (int64_t i = 1; i < n; ++i)
        if (counts[i] > counts[first]) first = i;
    for (int c = 0; c < 3; ++c) C[c] = P[3 * (size_t)first + c];
    for (int j = 1; j < K; ++j) {
        uint64_t best = 0;
        int64_t at = -1;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t d = okfit_dist(&P[3 * (size_t)i], &C[3 * (size_t)(j - 1)]);
            if (j == 1 || d < dist[i]) dist[i] = d;
            const uint64_t prod = (uint64_t)counts[i] * (uint64_t)dist[i];
            if (at < 0 || prod > best) best = prod, at = i;
        }
        for (int c = 0; c < 3; ++c) C[3 * (size_t)j + c] = best > 0 ? P[3 * (size_t)at + c] : C[c];
    }
    // Lloyd
    int n_iter = 0;
    for (int it = 0; it < max_iter; ++it) {
        ++n_iter;
        okfit_assign(P.data(), n, C.data(), K, labels.data(), dist.data());
        std::fill(S.begin(), S.end(), 0);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t i = 0; i < n; ++i) {
            const size_t k = (size_t)labels[i];
            cnt[k] += counts[i];
            for (int c = 0; c < 3; ++c) S[3 * k + c] += (int64_t)counts[i] * P[3 * (size_t)i + c];
        }
        bool changed = false;
        for (int k = 0; k < K; ++k) {
            if (!cnt[k]) continue;
            for (int c = 0; c < 3; ++c) {
                const int32_t v = (int32_t)okfit_floordiv(2 * S[3 * (size_t)k + c] + (int64_t)cnt[k], 2 * (int64_t)cnt[k]);
                changed |= v != C[3 * (size_t)k + c];
                C[3 * (size_t)k + c] = v;
            }
        }
        if (!changed) break;
    }
    // back to bytes
    okfit_assign(P.data(), n, C.data(), K, labels.data(), dist.data());
    std::vector<int64_t> near((size_t)K, -1);
    uint64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        const size_t k = (size_t)labels[i];
        total += (uint64_t)counts[i] * (uint64_t)dist[i];
        if (near[k] < 0 || dist[i] < dist[(size_t)near[k]]) near[k] = i;
    }
    for (int k = 0; k < K; ++k) {
        int64_t at = near[(size_t)k];
        if (at < 0) {
            int64_t best = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t d = okfit_dist(&P[3 * (size_t)i], &C[3 * (size_t)k]);
                if (at < 0 || d < best) best = d, at = i;
            }
        }
        palette[3 * k] = (uint8_t)(codes[at] >> 16);
        palette[3 * k + 1] = (uint8_t)(codes[at] >> 8);
        palette[3 * k + 2] = (uint8_t)codes[at];
        for (int c = 0; c < 3; ++c) centres[3 * k + c] = C[3 * (size_t)k + c];
    }
    *n_iter_out = n_iter;
    *distortion_out = total;
}

// ---- Filtered resize: coefficients, plan and the host statement (resample.hip, include/ditherpie_hip_resample.h) ------------
// Pillow's Image.resize for RGB uint8 frames, bit for bit: precompute_coeffs + normalize_coeffs_8bpc per axis, then the
// horizontal pass over the source rows the vertical pass needs into a uint8 intermediate, then the vertical pass.  float64 in
// the order of the header's definition (this file is compiled with -ffp-contract=off); everything after the coefficients is
// integer.  tests/resample_ref.py states the same in numpy.
constexpr int kResampleFilters = 5;        // DP_RESAMPLE_BOX .. DP_RESAMPLE_LANCZOS
constexpr int kResampleMaxSize = 16384;    // every size of a plan lies in 1 .. this
constexpr int kResampleBits = 22;          // coefficients in 1 / 2^22
// horizontal kernels (ResamplePlanHost::h_kernel): a lane per output pixel reading global memory, or a block of source rows
// staged in LDS with a lane per row (resample.hip)
enum { kResampleHNaive = 0, kResampleHStaged = 1 };
constexpr int kResampleStageRows = 64;     // rows of a staged block: one per lane of its single wave
constexpr int kResampleStageCols = 16;     // output columns a staged block walks
constexpr int kResampleStagePitch = 239;   // most dwords per staged row (odd: lane = row is conflict-free): 956 source bytes, 64 rows + the results < 64 KiB

inline double resample_support(const int filter)
{
    static const double s[kResampleFilters] = {0.5, 1.0, 1.0, 2.0, 3.0};
    return s[filter];
}

inline double resample_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return std::sin(x) / x;
}

inline double resample_filter(const int filter, double x)
{
    switch (filter) {
    case 0:   // box
        return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case 1:   // bilinear
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case 2:   // hamming
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * 3.14159265358979323846;
        return std::sin(x) / x * (0.54 + 0.46 * std::cos(x));
    case 3: {   // bicubic, a = -0.5
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default:   // lanczos
        if (-3.0 <= x && x < 3.0) return resample_sinc(x) * resample_sinc(x / 3);
        return 0.0;
    }
}

// One axis: bounds = (first source position, count) per output position, kk = ksize int32 coefficients per output position
// (zeros behind the count).  -> ksize.  The caller has checked 1 <= in, out <= kResampleMaxSize and the filter.
inline int resample_coeffs(const int in, const int out, const int filter, std::vector<int32_t> &bounds, std::vector<int32_t> &kk)
{
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double sup = resample_support(filter) * fs;
    const double ss = 1.0 / fs;
    const int ksize = (int)std::ceil(sup) * 2 + 1;
    bounds.assign(2 * (size_t)out, 0);
    kk.assign((size_t)out * (size_t)ksize, 0);
    std::vector<double> wbuf((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - sup + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + sup + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double wv = resample_filter(filter, (x + xmin - center + 0.5) * ss);
            wbuf[(size_t)x] = wv;
            ww += wv;
        }
        int32_t *k = &kk[(size_t)xx * (size_t)ksize];
        for (int x = 0; x < xmax; ++x) {
            double wv = wbuf[(size_t)x];
            if (ww != 0.0) wv /= ww;
            k[x] = wv < 0 ? (int32_t)(-0.5 + wv * (double)(1 << kResampleBits)) : (int32_t)(0.5 + wv * (double)(1 << kResampleBits));
        }
        bounds[2 * (size_t)xx] = xmin;
        bounds[2 * (size_t)xx + 1] = xmax;
    }
    return ksize;
}

struct ResampleAxis {
    int in = 0, out = 0, ksize = 0;
    std::vector<int32_t> bounds, kk;
    int64_t max_abs = 0;   // max |k|
    int64_t max_sum = 0;   // max over the output positions of 255 * sum |k| + 2^21: what the int32 accumulator must hold
};

struct ResamplePlanHost {
    int filter = 0, h = 0, w = 0, oh = 0, ow = 0;
    ResampleAxis ver, hor;   // hor is empty when ow == w, ver's tables are kept even when oh == h (they give y0, y1)
    int y0 = 0, y1 = 0;      // the source rows the vertical pass reads: what the horizontal pass produces
    bool need_h = false, need_v = false;
    bool mul32 = false;      // max |k| >= 2^23: the products do not fit v_mad_i32_i24
    int h_kernel = kResampleHNaive;
};

inline void resample_axis(const int in, const int out, const int filter, ResampleAxis &a)
{
    a.in = in;
    a.out = out;
    a.ksize = resample_coeffs(in, out, filter, a.bounds, a.kk);
    a.max_abs = a.max_sum = 0;
    for (int xx = 0; xx < out; ++xx) {
        int64_t sum = 0;
        for (int x = 0; x < a.bounds[2 * (size_t)xx + 1]; ++x) {
            const int64_t v = a.kk[(size_t)xx * (size_t)a.ksize + (size_t)x], av = v < 0 ? -v : v;
            sum += av;
            if (av > a.max_abs) a.max_abs = av;
        }
        const int64_t need = 255 * sum + ((int64_t)1 << (kResampleBits - 1));
        if (need > a.max_sum) a.max_sum = need;
    }
}

// Does the staged kernel serve this plan at all: every group of kResampleStageCols output columns reads a source span that fits a
// staged row; a wider window (LANCZOS 400 -> 2) does not.
inline bool resample_h_fits(const ResampleAxis &hor)
{
    for (int c0 = 0; c0 < hor.out; c0 += kResampleStageCols) {
        const int c1 = std::min(hor.out, c0 + kResampleStageCols);
        int lo = hor.bounds[2 * (size_t)c0], hi = lo;
        for (int c = c0; c < c1; ++c) {
            lo = std::min(lo, hor.bounds[2 * (size_t)c]);
            hi = std::max(hi, hor.bounds[2 * (size_t)c] + hor.bounds[2 * (size_t)c + 1]);
        }
        // the block loads whole dwords from the first byte of column lo: 3 bytes of slack for the last one
        if ((int64_t)(hi - lo) * 3 + 3 > (int64_t)kResampleStagePitch * 4) return false;
    }
    return true;
}

// The planner's rule for the horizontal pass: the staged kernel where it fits AND the filter's support is at least 2 (BICUBIC,
// LANCZOS: every source pixel lies in 4 or 6 windows, so staging it once pays: 1.3 - 1.6 x faster than the naive kernel as
// measured); with BOX a source pixel lies in one window and there is nothing to reuse (measured: equal at 4K -> 1080p, 1.9 x and
// 5.8 x slower at 1080p -> 270 x 480 and -> 64 x 114), BILINEAR and HAMMING (two windows) are unmeasured and stay naive.
inline int resample_h_kernel(const ResampleAxis &hor, const int filter)
{
    return resample_support(filter) >= 2.0 && resample_h_fits(hor) ? kResampleHStaged : kResampleHNaive;
}

// -> 0, or the rule broken: 1 a filter outside 0 .. 4, 2 a size outside 1 .. 16384 or h * w > 2^30, 3 the int32 sum of a pass
// could overflow (Pillow's would too)
inline int resample_plan(const int filter, const int h, const int w, const int oh, const int ow, ResamplePlanHost &p)
{
    p = ResamplePlanHost{};
    if (filter < 0 || filter >= kResampleFilters) return 1;
    if (h < 1 || w < 1 || oh < 1 || ow < 1 || h > kResampleMaxSize || w > kResampleMaxSize || oh > kResampleMaxSize || ow > kResampleMaxSize ||
        (int64_t)h * w > ((int64_t)1 << 30))
        return 2;
    p.filter = filter;
    p.h = h, p.w = w, p.oh = oh, p.ow = ow;
    p.need_h = ow != w;
    p.need_v = oh != h;
    resample_axis(h, oh, filter, p.ver);
    p.y0 = p.ver.bounds[0];
    p.y1 = p.ver.bounds[2 * (size_t)(oh - 1)] + p.ver.bounds[2 * (size_t)(oh - 1) + 1];
    int64_t max_abs = 0, max_sum = 0;
    if (p.need_v) max_abs = p.ver.max_abs, max_sum = p.ver.max_sum;
    if (p.need_h) {
        resample_axis(w, ow, filter, p.hor);
        max_abs = std::max(max_abs, p.hor.max_abs);
        max_sum = std::max(max_sum, p.hor.max_sum);
        p.h_kernel = resample_h_kernel(p.hor, filter);
    }
    if (max_sum >= ((int64_t)1 << 31)) return 3;
    p.mul32 = max_abs >= ((int64_t)1 << 23);
    return 0;
}

// one pass along an axis: `lines` lines of `len_out` pixels each; a pixel of line l at position x sits at l * line_stride +
// x * pos_stride (bytes, 3 channels there)
inline void resample_pass(const uint8_t *src, uint8_t *dst, const ResampleAxis &a, const int shift, const int64_t lines, const int64_t src_line,
                          const int64_t src_pos, const int64_t dst_line, const int64_t dst_pos)
{
    for (int64_t l = 0; l < lines; ++l)
        for (int xx = 0; xx < a.out; ++xx) {
            const int xmin = a.bounds[2 * (size_t)xx] - shift, cnt = a.bounds[2 * (size_t)xx + 1];
            const int32_t *k = &a.kk[(size_t)xx * (size_t)a.ksize];
            for (int c = 0; c < 3; ++c) {
                int64_t s = (int64_t)1 << (kResampleBits - 1);   // (a plan's sums fit int32; the wider type costs nothing here)
                for (int x = 0; x < cnt; ++x) s += (int64_t)src[l * src_line + (int64_t)(xmin + x) * src_pos + c] * k[x];
                s >>= kResampleBits;
                dst[l * dst_line + (int64_t)xx * dst_pos + c] = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
            }
        }
}

// The whole resize of n frames on the CPU: the statement the kernels are tested against
inline void resample_host(const ResamplePlanHost &p, const uint8_t *in, uint8_t *out, const int64_t n)
{
    const size_t fin = 3 * (size_t)p.h * (size_t)p.w, fout = 3 * (size_t)p.oh * (size_t)p.ow;
    std::vector<uint8_t> mid;
    if (p.need_h && p.need_v) mid.resize(3 * (size_t)(p.y1 - p.y0) * (size_t)p.ow);
    for (int64_t f = 0; f < n; ++f) {
        const uint8_t *src = in + (size_t)f * fin;
        uint8_t *dst = out + (size_t)f * fout;
        if (!p.need_h && !p.need_v) {
            std::memcpy(dst, src, fin);
        } else if (p.need_h && !p.need_v) {
            resample_pass(src, dst, p.hor, 0, p.h, 3 * (int64_t)p.w, 3, 3 * (int64_t)p.ow, 3);
        } else if (!p.need_h) {
            resample_pass(src, dst, p.ver, 0, p.w, 3, 3 * (int64_t)p.w, 3, 3 * (int64_t)p.w);
        } else {
            resample_pass(src + 3 * (size_t)p.y0 * (size_t)p.w, mid.data(), p.hor, 0, p.y1 - p.y0, 3 * (int64_t)p.w, 3, 3 * (int64_t)p.ow, 3);
            resample_pass(mid.data(), dst, p.ver, p.y0, p.ow, 3, 3 * (int64_t)p.ow, 3, 3 * (int64_t)p.ow);
        }
    }
}

// ---- temporal hold (include/ditherpie_hip_hold.h; tests/hold_ref.py states it in numpy) ---------------------------------------
constexpr int kHoldMaxCell = 16;
constexpr int64_t kHoldMaxFrames = 65535;

// -> 0, or the rule broken by the scalars of a hold call: 1 n_frames < 0, 2 h or w < 1 or h * w >= 2^31, 3 a cell that is none of
// 1, 2, 4, 8, 16, 4 tol outside 0 .. 255, 5 share256 outside 0 .. 256, 6 more than 65535 frames
inline int hold_rule(const int64_t n, const int h, const int w, const int cell, const int tol, const int share256)
{
    if (n < 0) return 1;
    if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return 2;
    if (cell < 1 || cell > kHoldMaxCell || (cell & (cell - 1))) return 3;
    if (tol < 0 || tol > 255) return 4;
    if (share256 < 0 || share256 > 256) return 5;
    if (n > kHoldMaxFrames) return 6;
    return 0;
}

// does a cell of cell_px pixels, `changed` of them changed, refresh?  (the one line the kernels and the statement share: constexpr,
// so device code may call it)
constexpr bool hold_refreshes(const uint32_t changed, const uint32_t cell_px, const uint32_t share256)
{
    return changed > 0 && changed * 256u >= share256 * cell_px;
}

// The statement: n frames in order, the state carried in anchor / held (not read when has_state is 0)
inline void hold_apply(const uint8_t *src, const uint8_t *planes, const int64_t n, const int h, const int w, const int cell, const int tol,
                       const int share256, uint8_t *anchor, uint8_t *held, const bool has_state, uint8_t *out, int64_t *refreshed)
{
    const size_t px = (size_t)h * (size_t)w;
    for (int64_t f = 0; f < n; ++f) {
        const uint8_t *s = src + (size_t)f * px * 3u;
        const uint8_t *p = planes + (size_t)f * px;
        int64_t count = 0;
        for (int y0 = 0; y0 < h; y0 += cell)
            for (int x0 = 0; x0 < w; x0 += cell) {
                const int y1 = std::min(h, y0 + cell), x1 = std::min(w, x0 + cell);
                const uint32_t cell_px = (uint32_t)(y1 - y0) * (uint32_t)(x1 - x0);
                bool refresh = true;
                if (has_state || f > 0) {
                    uint32_t changed = 0;
                    for (int y = y0; y < y1; ++y)
                        for (int x = x0; x < x1; ++x) {
                            const size_t i = ((size_t)y * (size_t)w + (size_t)x) * 3u;
                            int d = 0;
                            for (int c = 0; c < 3; ++c) d = std::max(d, std::abs((int)s[i + c] - (int)anchor[i + c]));
                            changed += d > tol ? 1u : 0u;
                        }
                    refresh = hold_refreshes(changed, cell_px, (uint32_t)share256);
                }
                if (!refresh) continue;
                count += cell_px;
                for (int y = y0; y < y1; ++y) {
                    const size_t i = (size_t)y * (size_t)w + (size_t)x0;
                    std::memcpy(anchor + i * 3u, s + i * 3u, 3u * (size_t)(x1 - x0));
                    std::memcpy(held + i, p + i, (size_t)(x1 - x0));
                }
            }
        std::memcpy(out + (size_t)f * px, held, px);
        refreshed[f] = count;
    }
}

// ---- transparency (include/ditherpie_hip_alpha.h; tests/alpha_ref.py states it in numpy) ---------------------------------------
constexpr int64_t kAlphaMaxFrames = 65535;
constexpr int kAlphaMaxOrigin = 1 << 30;

// -> 0, or the rule broken by the geometry of an alpha call: 1 n_frames < 0, 2 h or w < 1 or h * w >= 2^31, 3 more than 65535 frames
inline int alpha_geometry_rule(const int64_t n, const int h, const int w)
{
    if (n < 0) return 1;
    if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return 2;
    if (n > kAlphaMaxFrames) return 3;
    return 0;
}

// -> 0, or the rule broken by the settings of a split: 4 a mode that is neither, 5 a threshold outside 0 .. 256, 6 an m that is none
// of 2, 4, 8, 7 a y0 or x0 outside 0 .. 2^30.  Only the fields of the mode are looked at
inline int alpha_split_rule(const int mode, const int threshold, const int m, const int y0, const int x0)
{
    if (mode != 0 && mode != 1) return 4;
    if (mode == 0) return threshold < 0 || threshold > 256 ? 5 : 0;
    if (m != 2 && m != 4 && m != 8) return 6;
    if (y0 < 0 || y0 > kAlphaMaxOrigin || x0 < 0 || x0 > kAlphaMaxOrigin) return 7;
    return 0;
}

// B_m[y mod m][x mod m] for m = 1 << bits (the rank matrix of cells_bayer_rank); constexpr, so device code may call it
constexpr uint32_t alpha_bayer_rank(const int bits, const uint32_t y, const uint32_t x)
{
    uint32_t r = 0;
    for (int j = 0; j < bits; ++j) {
        const uint32_t yb = (y >> j) & 1u, xb = (x >> j) & 1u;
        r |= (((xb ^ yb) << 1) | yb) << (2 * (bits - 1 - j));
    }
    return r;
}

// is the pixel at global (gy, gx) with this alpha transparent?  bits: 0 for DP_ALPHA_THRESHOLD, else log2 m of DP_ALPHA_ORDERED
constexpr bool alpha_masked(const int bits, const uint32_t threshold, const uint32_t alpha, const uint32_t gy, const uint32_t gx)
{
    return bits == 0 ? alpha < threshold : (2u << (2 * bits)) * alpha < 255u * (2u * alpha_bayer_rank(bits, gy, gx) + 1u);
}

// a channel over the matte: (c alpha + M (255 - alpha) + 127) / 255
constexpr uint32_t alpha_matte(const uint32_t c, const uint32_t alpha, const uint32_t matte)
{
    return (c * alpha + matte * (255u - alpha) + 127u) / 255u;
}

constexpr int alpha_bits(const int mode, const int m) { return mode == 0 ? 0 : (m == 8 ? 3 : (m == 4 ? 2 : 1)); }

// The statements behind the _host_ entry points
inline void alpha_split(const uint8_t *rgba, const int64_t n, const int h, const int w, const int mode, const int threshold, const int m,
                        const int y0, const int x0, const bool has_matte, const uint8_t *matte, uint8_t *rgb, uint8_t *mask, int64_t *masked)
{
    const int bits = alpha_bits(mode, m);
    const size_t px = (size_t)h * (size_t)w;
    for (int64_t f = 0; f < n; ++f) {
        int64_t count = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)f * px + (size_t)y * (size_t)w + (size_t)x;
                const uint32_t a = rgba[4 * i + 3];
                for (int c = 0; c < 3; ++c) rgb[3 * i + c] = has_matte ? (uint8_t)alpha_matte(rgba[4 * i + c], a, matte[c]) : rgba[4 * i + c];
                const bool t = alpha_masked(bits, (uint32_t)threshold, a, (uint32_t)y0 + (uint32_t)y, (uint32_t)x0 + (uint32_t)x);
                mask[i] = t ? 1 : 0;
                count += t ? 1 : 0;
            }
        masked[f] = count;
    }
}

inline void alpha_key(const uint8_t *planes, const uint8_t *mask, const size_t px, const int key, uint8_t *out)
{
    for (size_t i = 0; i < px; ++i) out[i] = mask[i] ? (uint8_t)key : planes[i];
}

inline void alpha_join(const uint8_t *rgb, const uint8_t *mask, const size_t px, const uint8_t *fill, uint8_t *rgba)
{
    for (size_t i = 0; i < px; ++i) {
        for (int c = 0; c < 3; ++c) rgba[4 * i + c] = mask[i] ? fill[c] : rgb[3 * i + c];
        rgba[4 * i + 3] = mask[i] ? 0 : 255;
    }
}

}  // namespace dp
