// Candidate tables of the diffusion kernels (ediff.hip / vardiff.hip): everything that happens on the host between the
// download of ed_cells_kernel's geometric lists and the upload of the finished tables.  Pure C++17, no HIP headers; part of
// host_logic.h (which includes it) and compiled with it under the CPU sanitizers.
//
// Two entry points, one per caller:  ed_tables_build -- the tables every diffusion kernel searches (the 8^3 lists sharpened in
// place, their octree, the 16^3 lists, the hierarchical table, the nibble tables) -- and  ed_ext_build -- the extended 16^3 lists
// of the unclamped diffusers, built when such a diffuser first meets the palette so that plain error diffusion does not pay for
// them (5-16 ms).  Every table is a pure function of the palette (and of the kernel's lists); tests/golden/ed_tables_digests.json
// pins their bytes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <thread>
#include <utility>
#include <vector>

namespace dp {

struct U4 {  // layout of HIP's uint4
    uint32_t x, y, z, w;
};
inline U4 make_u4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return U4{x, y, z, w}; }

constexpr int kEdCells = 32 * 32 * 32;

// The per-cell loops below are independent: split them over a few host threads (the tables of a new palette are built
// at its first diffusion call, i.e. in front of a user's image).  Each thread writes only the cells of its own range.
template <class F>
inline void parallel_cells(const int n, F &&body, const int serial_below = 1024)
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 8 ? 8 : nt);
    if (n < serial_below || nt == 1) {
        body(0, n);
        return;
    }
    std::vector<std::thread> th;
    const int chunk = (n + (int)nt - 1) / (int)nt;
    for (unsigned t = 1; t < nt; ++t) {
        const int lo = (int)t * chunk, hi = std::min(n, lo + chunk);
        if (lo < hi) th.emplace_back([&body, lo, hi]() { body(lo, hi); });
    }
    body(0, std::min(n, chunk));
    for (auto &t : th) t.join();
}

struct EdTables {
    std::vector<U4> nodes;         // refinement of overflowing 8^3 cells (8 entries per node); empty if none
    std::vector<U4> l16;           // K > 16: lists of the 16^3 cells in the 8^3 table's format
    std::vector<uint32_t> coarse;  // K <= 16: lists of the 16^3 cells, count | 7 index nibbles
    std::vector<uint32_t> ext;     // K <= 16: the same over the extended grid (outermost cells = half-spaces)
    std::vector<U4> ext16;         // K > 16: l16 with the OUTERMOST cells standing for everything beyond them (unbounded boxes), for
                                   // the diffusers that do not clamp their values (vardiff.hip: nearest_ext16); count 255: too long
    std::vector<U4> ext_nodes;     // ... and the octree below the outermost cells whose list is too long (count 254 | node << 8: eight
                                   // half-size children, the outer ones unbounded again), at most kEdExtMaxNodes nodes
    // 17..256 colours: the hierarchical nearest table of at most four entries per leaf (ed_nearest.hip.h: nearest_h4).  Words [0, 4096):
    // the 16^3 cells; then nodes of 8 words: the 8-wide children of a cell, the 4-wide children of a child, the 2-wide ones of those.
    // A LEAF word holds four palette indices, byte 0 < byte 1 (listed entries, then an unlisted far entry as padding); a word with
    // byte 0 >= byte 1 is a MARKER: 0x00ff | node << 16 (node 0xffff: no answer here, use the lists).  Empty when it would not
    // fit kEdH4MaxWords.
    std::vector<uint32_t> h4;
    size_t h4_wanted = 0;          // words the table would take (reported by the experiments build)
    double h4_none = 0.0;          // fraction of the palette's own colours at which the table has no answer
    double h4_depth = 0.0;         // mean number of descents of nearest_h4 at the palette's own colours (4 = no answer): where a
                                   // palette puts its colours is where its images put their pixels
};
constexpr size_t kEdH4LdsWords = 27648;   // 108 KB: all the LDS the few-frames diffusion kernel has left (256 random colours: 21 336 words, median cut 256 of smooth content: 25 120)
constexpr size_t kEdH4MaxWords = 65536;   // largest table built (256 KB, node numbers stay below 0xffff): beyond the LDS size it is read from L2
constexpr uint32_t kEdH4NoAnswer = 0xffff00ffu;
constexpr size_t kEdExtMaxNodes = 2048;   // refinement nodes of the extended 16^3 lists (8 entries each: 256 KB)
// An 8^3 cell refined down to unit cubes has 1 + 8 + 64 nodes, so no palette overflows the node pointers of the 8^3 octree.
static_assert(73 * (size_t)kEdCells < (1u << 24), "the 8^3 octree's node numbers fit their 24-bit field");

// A list block (8^3 cells, their octree nodes, 16^3 cells): word 0's low byte is the count (254: node pointer in the upper 24 bits,
// 255: too long -- scan the palette), then the entries' palette indices: one BYTE each (up to 15) for palettes of up to 256 colours,
// TEN BITS each from bit 8 on (up to 12: 8 + 120 = 128 bits) for 257..1024 colours ("wide": without lists, error diffusion with
// more than 256 colours ran the KD-tree query at every pixel step: 0.44 s per 4K frame at 1024 colours).
inline int ed_list_cap(const int K) { return K > 256 ? 12 : 15; }
inline int ed_list_get(const uint32_t (&w)[4], const int pos /* 0-based */, const bool wide)
{
    if (!wide) return (int)((w[(pos + 1) >> 2] >> (8 * ((pos + 1) & 3))) & 255u);
    const int off = 8 + 10 * pos, wi = off >> 5, sh = off & 31;
    uint32_t v = w[wi] >> sh;
    if (sh > 22 && wi < 3) v |= w[wi + 1] << (32 - sh);
    return (int)(v & 1023u);
}
inline void ed_list_put(uint32_t (&w)[4], const int pos /* 0-based */, const int j, const bool wide)
{
    if (!wide) {
        w[(pos + 1) >> 2] |= (uint32_t)j << (8 * ((pos + 1) & 3));
        return;
    }
    const int off = 8 + 10 * pos, wi = off >> 5, sh = off & 31;
    w[wi] |= (uint32_t)j << sh;
    if (sh > 22 && wi < 3) w[wi + 1] |= (uint32_t)j >> (32 - sh);
}
constexpr U4 kEdScan = {255u, 0u, 0u, 0u};   // a list block without a list: scan the palette

// What every builder reads of the palette.  pts: K*3 float64 coordinates (not owned).
struct EdPalette {
    const double *pts;
    int K;
    bool wide;               // ten-bit list entries
    int cap;                 // entries a list block holds
    int corner_entry[8];     // the entry nearest to each corner of the cube: bit d of the index set = the corner's coordinate d is 255
    std::vector<int> all;    // 0 .. K-1
};
inline EdPalette ed_palette(const double *pts, const int K)
{
    EdPalette pal{pts, K, K > 256, ed_list_cap(K), {}, std::vector<int>((size_t)K)};
    for (int j = 0; j < K; ++j) pal.all[(size_t)j] = j;
    for (int c = 0; c < 8; ++c) {
        double best = std::numeric_limits<double>::infinity();
        pal.corner_entry[c] = 0;
        for (int j = 0; j < K; ++j) {
            double d2 = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double m = pts[3 * j + d] - ((c >> d) & 1 ? 255.0 : 0.0);
                d2 += m * m;
            }
            if (d2 < best) {
                best = d2;
                pal.corner_entry[c] = j;
            }
        }
    }
    return pal;
}

// An axis-aligned box of the colour cube.  [lo, lo + size]: its bounded part, where the clamped coordinates of its points fall;
// [blo, bhi]: the box itself -- the same, or with infinite sides where an outermost cell stands for everything beyond it.
struct EdBox {
    double lo[3], size, blo[3], bhi[3];
    // cell of the (1 << bits)^3 grid; open: the outermost cells are unbounded outwards
    static EdBox cell(const int cell, const int bits, const bool open = false)
    {
        constexpr double kInf = std::numeric_limits<double>::infinity();
        EdBox b;
        b.size = (double)(256 >> bits);
        for (int d = 0; d < 3; ++d) {
            const int last = (1 << bits) - 1, c = (cell >> (bits * d)) & last;
            b.lo[d] = (double)c * b.size;
            b.blo[d] = open && c == 0 ? -kInf : b.lo[d];
            b.bhi[d] = open && c == last ? kInf : b.lo[d] + b.size;
        }
        return b;
    }
    // half-size child: bit d of `sub` = the upper half along d; an infinite side stays with the children that touch it
    EdBox child(const int sub) const
    {
        constexpr double kInf = std::numeric_limits<double>::infinity();
        EdBox c;
        c.size = size * 0.5;
        for (int d = 0; d < 3; ++d) {
            const int bit = (sub >> d) & 1;
            c.lo[d] = lo[d] + (bit ? c.size : 0.0);
            c.blo[d] = (!bit && blo[d] == -kInf) ? -kInf : c.lo[d];
            c.bhi[d] = (bit && bhi[d] == kInf) ? kInf : c.lo[d] + c.size;
        }
        return c;
    }
    double centre(const int d) const { return lo[d] + 0.5 * size; }
    // squared distance from p to the bounded part
    double near2(const double *p) const
    {
        double d2 = 0.0;
        for (int d = 0; d < 3; ++d) {
            const double m = std::max(std::max(lo[d] - p[d], p[d] - (lo[d] + size)), 0.0);
            d2 += m * m;
        }
        return d2;
    }
};

struct EdScratch {   // per thread, reused from cell to cell
    std::vector<int> geo, list, tried;
    std::vector<std::pair<double, int>> order;
};

// The geometric criterion (as ed_cells_kernel applies it): the entries of `from` that are no farther from the box's bounded part than
// the nearest of them can be from any of its points.
inline void box_list(const EdPalette &pal, const EdBox &box, const std::vector<int> &from, std::vector<int> &list)
{
    double bound = std::numeric_limits<double>::infinity();
    for (int j : from) {
        double far2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double c = pal.pts[3 * j + k];
            const double m = std::max(std::fabs(c - box.lo[k]), std::fabs(c - (box.lo[k] + box.size)));
            far2 += m * m;
        }
        bound = std::min(bound, far2);
    }
    bound = bound * (1.0 + 1e-12) + 1e-9;
    list.clear();
    for (int j : from)
        if (box.near2(pal.pts + 3 * j) <= bound) list.push_back(j);
}

// k is closer than j to EVERY point of the box, i.e. the box lies strictly on k's side of the bisector of j and k:
//   max over the box of |x - c_k|^2 - |x - c_j|^2 = max of 2 x.(c_j - c_k) + |c_k|^2 - |c_j|^2 < 0   (linear in x).
// kOpen: the box may have infinite sides (over one in a direction in which the difference grows the maximum is +inf: k cannot be;
// 0 * inf must not arise).  Bounded boxes take the form without data-dependent branches: this is the innermost loop of every table.
template <bool kOpen>
inline bool ed_dominates(const EdPalette &pal, const EdBox &box, const int k, const int j)
{
    const double *pj = pal.pts + 3 * j, *pk = pal.pts + 3 * k;
    double mx = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double a = 2.0 * (pj[d] - pk[d]);
        if (kOpen) mx += a > 0.0 ? a * box.bhi[d] : a < 0.0 ? a * box.blo[d] : 0.0;
        else mx += std::max(a * box.blo[d], a * box.bhi[d]);
        mx += pk[d] * pk[d] - pj[d] * pj[d];
    }
    return mx < -1e-9 * (1.0 + std::fabs(mx));
}
// A sharper (still conservative) list for a box: the entries of `from`, in their order, that no other entry of `from` dominates.  The
// true nearest entry of a point of the box is dominated by nobody, so it stays listed, with everything tied with it.
// kNearestFirst: the candidates k are tried nearest to the box's bounded part first (s.order[0].first: that distance, squared) --
// the same list, sooner where `from` is long (most entries fall to one of the first few), at the price of a sort.
template <bool kOpen, bool kNearestFirst>
inline void undominated(const EdPalette &pal, const EdBox &box, const std::vector<int> &from, std::vector<int> &list, EdScratch &s)
{
    if (kNearestFirst) {
        s.order.clear();
        for (int j : from) s.order.emplace_back(box.near2(pal.pts + 3 * j), j);
        std::sort(s.order.begin(), s.order.end());
        s.tried.clear();
        for (const std::pair<double, int> &o : s.order) s.tried.push_back(o.second);
    }
    const std::vector<int> &tried = kNearestFirst ? s.tried : from;
    list.clear();
    for (int j : from) {
        bool dominated = false;
        for (int k : tried)
            if (k != j && ed_dominates<kOpen>(pal, box, k, j)) {
                dominated = true;
                break;
            }
        if (!dominated) list.push_back(j);
    }
}
// both criteria: what a bounded box lists of `from`
inline void box_candidates(const EdPalette &pal, const EdBox &box, const std::vector<int> &from, std::vector<int> &list, EdScratch &s)
{
    box_list(pal, box, from, s.geo);
    undominated<false, false>(pal, box, s.geo, list, s);
}

// The filler of a list's unused positions: an entry that is NOT on the list and far from the box.  The key scans of the kernels
// evaluate whole groups of positions without per-position tests; an unlisted entry is never the nearest of a point of the box, and
// should float32 rounding bring it within the margin of the nearest, the exact scan -- which honours the count -- decides.
// Centre: the farthest from the box's centre; CornerOrCentre: the entry nearest to the cube corner opposite to the box unless that
// one is listed (any unlisted entry will do; this one needs no scan); Box: the farthest from the box.  -1: every entry is listed.
enum class EdFar { Centre, CornerOrCentre, Box };
inline int far_unlisted(const EdPalette &pal, const EdBox &box, const std::vector<int> &list, const EdFar rule)
{
    auto listed = [&](const int j) { return std::find(list.begin(), list.end(), j) != list.end(); };
    if (rule == EdFar::CornerOrCentre) {
        const int oct = (box.centre(0) < 128.0 ? 1 : 0) | (box.centre(1) < 128.0 ? 2 : 0) | (box.centre(2) < 128.0 ? 4 : 0);
        if (!listed(pal.corner_entry[oct])) return pal.corner_entry[oct];
    }
    int filler = -1;
    double far_d = -1.0;
    for (int j = 0; j < pal.K; ++j) {
        if (listed(j)) continue;
        double d2 = 0.0;
        if (rule == EdFar::Box) {
            d2 = box.near2(pal.pts + 3 * j);
        } else {
            for (int d = 0; d < 3; ++d) {
                const double m = pal.pts[3 * j + d] - box.centre(d);
                d2 += m * m;
            }
        }
        if (d2 > far_d) {
            far_d = d2;
            filler = j;
        }
    }
    return filler;
}

// A list block: count byte + the entries.  Lists of up to 12 entries are padded to a multiple of 4 positions with far_unlisted.
inline U4 pack(const EdPalette &pal, const std::vector<int> &list, const EdBox &box)
{
    uint32_t w[4] = {(uint32_t)list.size(), 0u, 0u, 0u};
    for (size_t n = 0; n < list.size(); ++n) ed_list_put(w, (int)n, list[n], pal.wide);
    if (!list.empty() && list.size() <= 12 && (int)list.size() < pal.K) {
        const int filler = far_unlisted(pal, box, list, EdFar::CornerOrCentre);
        for (size_t n = list.size(); n < (list.size() + 3) / 4 * 4 && filler >= 0; ++n) ed_list_put(w, (int)n, filler, pal.wide);
    }
    return make_u4(w[0], w[1], w[2], w[3]);
}
// A leaf of the hierarchical table: the (at most four) listed entries, padded with the filler pack() would choose.
inline uint32_t h4_leaf(const EdPalette &pal, const std::vector<int> &list, const EdBox &box)
{
    const int filler = far_unlisted(pal, box, list, EdFar::CornerOrCentre);
    int b[4];
    for (int n = 0; n < 4; ++n) b[n] = n < (int)list.size() ? list[(size_t)n] : filler;
    // byte 0 < byte 1 marks a leaf: two distinct indices always exist (a list of one is padded with its filler)
    if (b[0] > b[1]) std::swap(b[0], b[1]);
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}
// A word of the nibble tables (K <= 16): count | up to 7 indices, the unused positions filled (K > 8 > list size: there is a
// filler); count 15: too long.
inline uint32_t nibble_word(const EdPalette &pal, const std::vector<int> &list, const EdBox &box, const EdFar rule)
{
    if (list.size() > 7) return 15u;
    uint32_t word = (uint32_t)list.size();
    for (size_t n = 0; n < list.size(); ++n) word |= (uint32_t)list[n] << (4 * (n + 1));
    const int filler = far_unlisted(pal, box, list, rule);
    for (size_t n = list.size(); n < 7 && filler >= 0; ++n) word |= (uint32_t)filler << (4 * (n + 1));
    return word;
}

// ---- the octrees: a box whose list is too long for a leaf becomes a node of its eight half-size children ------------------------
// Each top-level cell is refined on its own (in parallel) into a LOCAL array -- [0]: the cell's own word, then 8 words per node,
// pointers holding local node numbers -- and the arrays are joined afterwards.  Depth-first, children pushed 0..7 and popped
// last-first: the node order is part of the tables' bytes.
struct EdItem {
    size_t slot;             // where the box's word goes in the local array
    EdBox box;
    std::vector<int> from;   // the parent's list
};
// Policy: Word none (no list here), leaf_max, list(item, out) (how a box's list is made), leaf(list, box), may_split(item, node)
// (node: the number the new node would get), pointer(node).
template <class Word, class Policy>
inline void ed_octree(const EdBox &top, const std::vector<int> &from, Policy &p, std::vector<EdItem> &todo, std::vector<int> &list,
                      std::vector<Word> &out)
{
    out.assign(1, p.none);
    todo.clear();
    todo.push_back(EdItem{0, top, from});
    while (!todo.empty()) {
        EdItem it = std::move(todo.back());
        todo.pop_back();
        p.list(it, list);
        if (list.size() <= p.leaf_max) {
            out[it.slot] = p.leaf(list, it.box);
            continue;
        }
        const size_t node = (out.size() - 1) / 8;
        if (!p.may_split(it, node)) continue;
        out[it.slot] = p.pointer(node);
        out.resize(out.size() + 8, p.none);
        for (int sub = 0; sub < 8; ++sub) todo.push_back(EdItem{1 + 8 * node + (size_t)sub, it.box.child(sub), list});
    }
}
// node pointers of a local array made global: `base` = the global number of its node 0
inline U4 ed_rebase(U4 e, const size_t base)
{
    if ((e.x & 255u) == 254u) e.x = 254u | ((uint32_t)(base + (e.x >> 8)) << 8);
    return e;
}
inline bool h4_marker(const uint32_t w) { return (w & 0xffu) >= ((w >> 8) & 0xffu); }
inline uint32_t ed_rebase(const uint32_t w, const size_t base)
{
    return h4_marker(w) && w != kEdH4NoAnswer ? 0x00ffu | ((uint32_t)(base + (w >> 16)) << 16) : w;
}
// appends a local array's nodes to `nodes` and returns the cell's own word
template <class Word>
inline Word ed_join(const std::vector<Word> &local, const size_t base, std::vector<Word> &nodes)
{
    for (size_t i = 1; i < local.size(); ++i) nodes.push_back(ed_rebase(local[i], base));
    return ed_rebase(local[0], base);
}

struct EdListPolicy {   // the octrees of list blocks
    const EdPalette &pal;
    EdScratch &s;
    U4 none = kEdScan;
    size_t leaf_max;
    EdListPolicy(const EdPalette &p, EdScratch &sc) : pal(p), s(sc), leaf_max((size_t)p.cap) {}
    U4 leaf(const std::vector<int> &list, const EdBox &box) const { return pack(pal, list, box); }
    U4 pointer(const size_t node) const { return make_u4(254u | ((uint32_t)node << 8), 0u, 0u, 0u); }
};

// The kernel's 8^3 lists (count byte | entries, count 255 = overflow), sharpened by the pairwise test and padded.
inline void ed_sharpen_cells(const EdPalette &pal, std::vector<U4> &cells)
{
    parallel_cells(kEdCells, [&](const int c0, const int c1) {
        EdScratch s;
        for (int cell = c0; cell < c1; ++cell) {
            const uint32_t w4[4] = {cells[cell].x, cells[cell].y, cells[cell].z, cells[cell].w};
            const int n = (int)(w4[0] & 255u);
            if (n < 1 || n > pal.cap) continue;
            s.geo.clear();
            for (int i = 0; i < n; ++i) s.geo.push_back(ed_list_get(w4, i, pal.wide));
            const EdBox box = EdBox::cell(cell, 5);
            undominated<false, false>(pal, box, s.geo, s.list, s);
            cells[cell] = pack(pal, s.list, box);  // (re-packed even when nothing was dropped: the padding)
        }
    });
}

// The 8^3 cells whose geometric list overflowed: their full pruned lists and, where even those are too long, their octrees down
// to unit cubes (a unit cube that still sees too many entries: scan the palette).  In parallel: a crowded palette has hundreds of
// such cells, and a list of a hundred entries costs ten thousand pairwise tests.
inline void ed_refine_overflow(const EdPalette &pal, std::vector<U4> &cells, std::vector<U4> &nodes)
{
    struct Policy : EdListPolicy {
        using EdListPolicy::EdListPolicy;
        void list(const EdItem &it, std::vector<int> &out) { box_candidates(pal, it.box, it.from, out, s); }
        bool may_split(const EdItem &it, size_t) const { return it.box.size > 1.0; }
    };
    std::vector<int> over;
    for (int cell = 0; cell < kEdCells; ++cell)
        if ((cells[cell].x & 255u) == 255u) over.push_back(cell);
    std::vector<std::vector<U4>> local(over.size());
    parallel_cells((int)over.size(), [&](const int i0, const int i1) {
        EdScratch s;
        Policy policy(pal, s);
        std::vector<EdItem> todo;
        for (int i = i0; i < i1; ++i) ed_octree(EdBox::cell(over[(size_t)i], 5), pal.all, policy, todo, s.list, local[(size_t)i]);
    }, 16);
    nodes.clear();
    for (size_t i = over.size(); i-- > 0;) cells[(size_t)over[i]] = ed_join(local[i], nodes.size() / 8, nodes);   // (descending: part of the bytes)
}

// Lists of the 16x16x16 cells in the format of the 8x8x8 table, for the LDS of the wavefront kernel's few-frames variant (one
// wave per SIMD: the read of the 8x8x8 table from L2 is half of a step's latency there).  top16 (optional): the cells' lists
// themselves, whatever their length.
inline void ed_build_l16(const EdPalette &pal, std::vector<U4> &l16, std::vector<std::vector<int>> *top16)
{
    l16.resize(4096);
    if (top16) top16->assign(4096, std::vector<int>());
    parallel_cells(4096, [&](const int c0, const int c1) {
        EdScratch s;
        for (int cell = c0; cell < c1; ++cell) {
            std::vector<int> &list = top16 ? (*top16)[(size_t)cell] : s.list;
            const EdBox box = EdBox::cell(cell, 4);
            box_candidates(pal, box, pal.all, list, s);
            l16[cell] = (int)list.size() <= pal.cap ? pack(pal, list, box) : kEdScan;
        }
    });
}

// The extended table for query points that are NOT clamped to the cube (perceptual / hybrid / adaptive-variance diffusion): a
// point is looked up in the cell of its clamped coordinates, so an outermost cell stands for everything beyond it.  Over such an
// unbounded box the geometric criterion lists everybody; the pairwise test alone decides (without the table these diffusers scan
// the whole palette at every step: 59 ms per 1080p frame at 256 colours against 4.6 ms for plain error diffusion,
// tools/bench_scripts/cliff_hunt.py).  A cell whose list is too long (a palette crowded at a face of the cube -- every palette
// under use_gamma, at the dark end) is cut into its eight half-size children like the 8^3 cells are: an outer child stays unbounded
// on its outer side, a point beyond the cube falls into it by its clamped coordinates.
inline void ed_build_ext16(const EdPalette &pal, const std::vector<U4> &l16, std::vector<U4> &ext16, std::vector<U4> &ext_nodes)
{
    struct Policy : EdListPolicy {
        using EdListPolicy::EdListPolicy;
        double nearest2 = 0.0;   // squared distance from the box to the nearest entry of the parent's list
        void list(const EdItem &it, std::vector<int> &out)
        {
            undominated<true, true>(pal, it.box, it.from, out, s);
            nearest2 = s.order.empty() ? std::numeric_limits<double>::infinity() : s.order[0].first;
        }
        // Left to the whole-palette scan: unit boxes; more than 24 nodes in one cell; and cells far from every colour of the
        // palette -- error diffusion keeps its values near the palette, and it is exactly the far cells of a crowded palette, to
        // which all its colours look alike, that are expensive to refine: with them the tables of a 256-colour median-cut
        // palette took 77 ms instead of 17.
        bool may_split(const EdItem &it, const size_t node) const { return it.box.size > 1.0 && node < 24 && nearest2 <= 40.0 * 40.0; }
    };
    ext16 = l16;
    std::vector<int> shell;   // the outermost cells
    for (int cell = 0; cell < 4096; ++cell) {
        const int c0 = cell & 15, c1 = (cell >> 4) & 15, c2 = cell >> 8;
        if (c0 == 0 || c0 == 15 || c1 == 0 || c1 == 15 || c2 == 0 || c2 == 15) shell.push_back(cell);
    }
    std::vector<std::vector<U4>> local(shell.size());
    parallel_cells((int)shell.size(), [&](const int i0, const int i1) {
        EdScratch s;
        Policy policy(pal, s);
        std::vector<EdItem> todo;
        for (int i = i0; i < i1; ++i) ed_octree(EdBox::cell(shell[(size_t)i], 4, true), pal.all, policy, todo, s.list, local[(size_t)i]);
    }, 64);
    ext_nodes.clear();
    for (size_t i = 0; i < shell.size(); ++i) {
        const size_t base = ext_nodes.size() / 8;
        const bool room = base + (local[i].size() - 1) / 8 <= kEdExtMaxNodes;
        ext16[(size_t)shell[i]] = room ? ed_join(local[i], base, ext_nodes) : kEdScan;   // no room: scan
    }
}

// The hierarchical table: a wave of the diffusion kernel pays for the LONGEST list among its 64 lanes, and with 256 random
// colours 12 % of the 16^3 cells, 0.8 % of the 8-wide and 0.03 % of the 4-wide cells have more than four possible nearest
// entries -- so a cell with more than four is cut into its eight 8-wide children, such a child into its 4-wide children, those
// into 2-wide ones, and every lane ends at a leaf of at most four (what is still longer in a 2-wide box has no answer here: the
// lists decide).  top16: the 16^3 cells' lists (ed_build_l16).  Returns the words the table takes; h4 stays empty when that is
// more than fits (a clustered palette: the lists and their octree serve it).
inline size_t ed_build_h4(const EdPalette &pal, const std::vector<std::vector<int>> &top16, std::vector<uint32_t> &h4)
{
    struct Policy {
        const EdPalette &pal;
        EdScratch &s;
        const std::vector<int> *top;
        uint32_t none = kEdH4NoAnswer;
        size_t leaf_max = 4;
        void list(const EdItem &it, std::vector<int> &out)
        {
            if (it.slot == 0) out = *top;   // (both criteria over the whole palette: done for l16)
            else box_candidates(pal, it.box, it.from, out, s);
        }
        uint32_t leaf(const std::vector<int> &list, const EdBox &box) const { return h4_leaf(pal, list, box); }
        bool may_split(const EdItem &it, size_t) const { return it.box.size > 2.0; }
        uint32_t pointer(const size_t node) const { return 0x00ffu | ((uint32_t)node << 16); }
    };
    std::vector<std::vector<uint32_t>> local(4096);
    parallel_cells(4096, [&](const int c0, const int c1) {
        EdScratch s;
        Policy policy{pal, s, nullptr};
        std::vector<EdItem> todo;
        const std::vector<int> none;   // (the top box takes its list from top16)
        for (int cell = c0; cell < c1; ++cell) {
            policy.top = &top16[(size_t)cell];
            ed_octree(EdBox::cell(cell, 4), none, policy, todo, s.list, local[(size_t)cell]);
        }
    });
    size_t wanted = 0;
    for (const std::vector<uint32_t> &lw : local) wanted += lw.size();
    h4.assign(4096, kEdH4NoAnswer);
    for (int cell = 0; cell < 4096; ++cell) {
        const std::vector<uint32_t> &lw = local[(size_t)cell];
        const size_t base = (h4.size() - 4096) / 8;
        if (h4.size() + (lw.size() - 1) > kEdH4MaxWords || base + (lw.size() - 1) / 8 >= 0xffffu) {
            h4.clear();
            break;
        }
        const uint32_t top = ed_join(lw, base, h4);
        h4[(size_t)cell] = top;
    }
    return wanted;
}

// How deep nearest_h4 walks at the palette's own colours (EdTables::h4_depth, h4_none).
inline void ed_h4_stats(const EdPalette &pal, const std::vector<uint32_t> &h4, double &depth_mean, double &none_fraction)
{
    double total = 0.0, none = 0.0;
    for (int j = 0; j < pal.K; ++j) {
        uint32_t x[3];
        for (int d = 0; d < 3; ++d) x[d] = (uint32_t)std::min(255.0, std::max(0.0, std::floor(pal.pts[3 * j + d] + 0.5)));
        uint32_t w = h4[(x[0] >> 4) | ((x[1] >> 4) << 4) | ((x[2] >> 4) << 8)];
        int depth = 0;
        for (int bit = 3; bit >= 1 && h4_marker(w); --bit) {
            if ((w >> 16) == 0xffffu) break;
            w = h4[4096u + (size_t)(w >> 16) * 8u + (((x[0] >> bit) & 1u) | (((x[1] >> bit) & 1u) << 1) | (((x[2] >> bit) & 1u) << 2))];
            ++depth;
        }
        total += h4_marker(w) ? 4.0 : (double)depth;
        none += h4_marker(w) ? 1.0 : 0.0;
    }
    depth_mean = total / (double)pal.K;
    none_fraction = none / (double)pal.K;
}

// K <= 16: lists of the 16x16x16 cells for the wavefront kernel's LDS, one nibble per entry (nibble_word).
inline void ed_build_coarse(const EdPalette &pal, std::vector<uint32_t> &coarse)
{
    coarse.resize(4096);
    parallel_cells(4096, [&](const int c0, const int c1) {
        EdScratch s;
        for (int cell = c0; cell < c1; ++cell) {
            const EdBox box = EdBox::cell(cell, 4);
            box_candidates(pal, box, pal.all, s.list, s);
            coarse[cell] = nibble_word(pal, s.list, box, EdFar::Box);
        }
    });
}
// K <= 16: the same table for the unclamped diffusers, the outermost cells unbounded as in ed_build_ext16 (the pairwise test
// alone: 256 pairs per cell).
inline void ed_build_ext(const EdPalette &pal, std::vector<uint32_t> &ext)
{
    ext.resize(4096);
    parallel_cells(4096, [&](const int c0, const int c1) {
        EdScratch s;
        for (int cell = c0; cell < c1; ++cell) {
            const EdBox box = EdBox::cell(cell, 4, true);
            undominated<true, false>(pal, box, pal.all, s.list, s);
            ext[cell] = nibble_word(pal, s.list, box, EdFar::Centre);
        }
    });
}

// The tables every diffusion kernel uses.  cells [kEdCells]: in = the kernel's lists, out = sharpened, padded, the overflowing
// cells pointing into out.nodes.  Leaves out.ext16 / out.ext_nodes alone.
inline void ed_tables_build(const EdPalette &pal, std::vector<U4> &cells, EdTables &out)
{
    ed_sharpen_cells(pal, cells);
    ed_refine_overflow(pal, cells, out.nodes);
    out.l16.clear();
    out.coarse.clear();
    out.ext.clear();
    out.h4.clear();
    out.h4_wanted = 0;
    out.h4_depth = out.h4_none = 0.0;
    if (pal.K <= 16) {
        ed_build_coarse(pal, out.coarse);
        ed_build_ext(pal, out.ext);
        return;
    }
    std::vector<std::vector<int>> top16;
    ed_build_l16(pal, out.l16, pal.wide ? nullptr : &top16);
    if (pal.wide) return;   // (the leaves of h4 hold index BYTES)
    out.h4_wanted = ed_build_h4(pal, top16, out.h4);
    if (!out.h4.empty()) ed_h4_stats(pal, out.h4, out.h4_depth, out.h4_none);
}

// The extended 16^3 lists of the unclamped diffusers, 17..1024 colours: out.ext16 / out.ext_nodes, and out.l16, from which they
// start.  Touches nothing else of `out`.
inline void ed_ext_build(const EdPalette &pal, EdTables &out)
{
    out.ext16.clear();
    out.ext_nodes.clear();
    if (pal.K <= 16) return;
    ed_build_l16(pal, out.l16, nullptr);
    ed_build_ext16(pal, out.l16, out.ext16, out.ext_nodes);
}

}  // namespace dp
