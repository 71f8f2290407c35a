// Nearest palette entry of an arbitrary float32 point, as scipy's KD-tree query (k=1) reports it: float32 prefilter,
// float64 validation, tree replay for exact ties; optionally restricted to the candidate list of the point's cell
// (ediff.hip: build_ed_cells).  Where this search is written: the error-diffusion kernels (ediff.hip), the variable-weight
// diffusers (vardiff.hip) and the Riemersma walk (riemersma.hip) call it (one exception under "per-wave search" below).
//
//   building blocks   ed_key / ed_key_expanded, KeyTop2 (integer keys), Top2 (exact float32 distances), the cell index,
//                     one key scan and one exact scan per list format (nibble, byte, wide)
//   per-lane search   nearest_color (whole palette), nearest_color_cells (points of the cube), nearest_ext / nearest_ext16
//                     (any point: the extended tables), nearest_h4
//   per-wave search   wave_nearest + wave_nearest_record (the palette spread over the lanes of one wave: os_rowserial_kernel and
//                     riemersma_kernel.  ed_rowserial_kernel in ediff.hip keeps its own open-coded copy of the two -- with the
//                     helpers its 16-colour step, M = 1, measured 4 % slower twice in the same-process A/B, from nothing but
//                     which compare went through VCC and the polarity of two branches (profiles/HISTORY.md, last section): a
//                     change to the margin or the near-tie test here has to be made there as well)
#pragma once
#include "dp_internal.h"
#include "tree_query.hip.h"
#include "wave_util.hip.h"

namespace dp {
namespace {

constexpr float kEdInf = __builtin_huge_valf();

// Naming a candidate record's fourth word keeps its LDS read a ds_read_b128: four LDS cycles per wave (groups of 16 lanes
// over 64 banks), where the ds_read_b96 the compiler narrows a three-component use to takes eight (groups of 8 over 32
// banks; MI355X_MICROARCH.md, LDS).  Found on ordered_compact_float_kernel in round 3: 1.22 -> 0.94 ms from this alone.
__device__ __forceinline__ void keep_record_whole(const float4 &c) { asm volatile("" ::"v"(c.w)); }

// float32 squared distance of record `c` = {x, y, z, out_rgb bits} to the point -- a filter only: every caller allows for
// its rounding (|d_f32 - d| <= ~3.6e-7 d: one rounding per subtract, square and add) with a margin
__device__ __forceinline__ float ed_dist(const float4 c, const float o0, const float o1, const float o2)
{
    keep_record_whole(c);
    const float a = c.x - o0, b = c.y - o1, cc = c.z - o2;
    return __fmaf_rn(a, a, __fmaf_rn(b, b, cc * cc));
}

// That distance as an integer key (non-negative floats order like their bit patterns), the low TAG_BITS bits replaced by
// `tag`, the candidate's position on its list: 3 bits for the nibble lists and the H4 leaves, 4 for the byte and wide lists
template <int TAG_BITS>
__device__ __forceinline__ int ed_key(const float4 c, const float o0, const float o1, const float o2, const uint32_t tag)
{
    return (int)((__float_as_uint(ed_dist(c, o0, o1, o2)) & ~((1u << TAG_BITS) - 1u)) | tag);
}

// The same 3-bit key from a candidate's EXPANDED record {-2x, -2y, -2z, |c|^2 + 2^18} (ediff.hip, palettes of up to 16 colours):
// |c - o|^2 - |o|^2 + 2^18 in three fused multiply-adds, four instructions per candidate with the tag instead of seven.  The
// term |o|^2 is common to all candidates and the bias keeps the value inside [2^16, 2^19) for points of the cube -- positive,
// so the bit patterns order like the values, and with an ulp of at most 2^-5: one rounding of the fourth word (float
// palettes; integer ones are exact), one per multiply-add and up to 8 ulp from the tag bits are below 0.32 in absolute
// terms per key (ed_expanded_margin).  Only the EXPANDED instance of nearest_color_cells calls it, and only
// ed_wavefront_kernel (ediff.hip) instantiates that one, after clamping the point to [0, 255]: the variable-weight diffusers, whose
// points leave the cube, take the plain instance (the face, edge and corner queries of tests/test_gpu_steered_queries.py sit
// on that boundary).
__device__ __forceinline__ int ed_key_expanded(const float4 x, const float o0, const float o1, const float o2, const uint32_t tag)
{
    keep_record_whole(x);
    const float d = __fmaf_rn(x.x, o0, __fmaf_rn(x.y, o1, __fmaf_rn(x.z, o2, x.w)));
    return (int)((__float_as_uint(d) & ~7u) | tag);
}
constexpr float kEdExpandedBias = 262144.0f;
constexpr float kEdExpandedMargin = 0.75f;  // > 2 * 0.32: a second key this far above the first proves the float64 order

__device__ __forceinline__ int ed_med3(const int a, const int b, const int c)
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The two smallest of a stream of integer keys, without bookkeeping: 2 instructions per key, and the winner's list
// position comes back out of the tag bits of m0.
struct KeyTop2 {
    int m0 = 0x7fffffff, m1 = 0x7fffffff;
    __device__ __forceinline__ void first3(const int k1, const int k2, const int k3)  // (from the empty state)
    {
        m0 = min(min(k1, k2), k3);
        m1 = ed_med3(k1, k2, k3);
    }
    __device__ __forceinline__ void add(const int k)
    {
        m1 = ed_med3(m0, m1, k);
        m0 = min(m0, k);
    }
    // The second key is more than the factor `rel` above the first: 2e-6 (relative) for the float32 evaluation plus the
    // tag bits -- up to 7 ulp (8.4e-7) under 3-bit tags: 1.000003f, up to 15 ulp under 4-bit tags: 1.000004f.  Then the
    // float64 order is proven; otherwise an exact scan decides.  (The empty state is a NaN: never decided.)
    template <int TAG_BITS>
    __device__ __forceinline__ bool decided(const float rel) const
    {
        constexpr int mask = ~((1 << TAG_BITS) - 1);
        return __int_as_float(m1 & mask) > __int_as_float(m0 & mask) * rel;
    }
};

// Near ties of the float32 scans: the float64 scan over the whole palette with the KD-tree's arithmetic (pal.pts), and
// scipy's traversal replayed (tree_query, its heap CAP deep) on exact ties of palettes larger than a leaf.
template <int CAP>
__device__ __forceinline__ int nearest_f64(const PalDev &pal, const float o0, const float o1, const float o2)
{
    const double x0 = (double)o0, x1 = (double)o1, x2 = (double)o2;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double b0 = inf, b1 = inf;
    int i0 = 0;
    const int K = pal.K;
    for (int j = 0; j < K; ++j) {
        const double d = sq_dist3(pal.pts + 3 * j, x0, x1, x2);
        if (d < b0) {
            b1 = b0;
            b0 = d;
            i0 = j;
        } else if (d < b1) {
            b1 = d;
        }
    }
    if (b0 == b1 && K > kLeafSize) {
        double d2[1];
        int ii[1];
        tree_query<1, CAP>(pal, x0, x1, x2, d2, ii);
        i0 = ii[0];
    }
    return i0;
}

// An exact tie at an integer point of the cube, integer palette with tie codes (accel.hip): the float32 distances are
// exact there, and which of several entries at the smallest distance scipy's traversal reports is tabulated (k=1 code:
// 0 / 1 / 2 = the first / second / third of them in index order).  Flat image regions under the adaptive-variance gate
// are exactly this case (no error arrives, the query is the pixel itself), and lattice or image-derived palettes tie on
// 5-20 % of such pixels; the generic answer (float64 scan + traversal replay with its heaps in scratch memory) costs
// microseconds per occurrence.  `cand`: all pal.K records; b0, i0: the smallest float32 distance and the lowest index
// that has it.  Returns -1 when the shortcut does not apply or the code says "other".
__device__ __forceinline__ int integer_tie_choice(const PalDev &pal, const float4 *__restrict__ cand, const float o0,
                                                  const float o1, const float o2, const float b0, const int i0)
{
    if (!pal.is_integer || pal.code1 == nullptr) return -1;
    if (!(o0 >= 0.0f && o0 <= 255.0f && o1 >= 0.0f && o1 <= 255.0f && o2 >= 0.0f && o2 <= 255.0f)) return -1;
    const uint32_t r = (uint32_t)o0, g = (uint32_t)o1, b = (uint32_t)o2;
    if ((float)r != o0 || (float)g != o1 || (float)b != o2) return -1;
    const uint32_t x = r | (g << 8) | (b << 16);
    const uint32_t code = (pal.code1[x >> 4] >> ((x & 15u) * 2)) & 3u;
    if (code == 0u) return i0;  // the lowest index among the tied entries (candidates are visited in index order)
    if (code == 3u) return -1;
    uint32_t seen = 0;
    for (int j = 0; j < pal.K; ++j) {
        const float4 c = cand[j];
        const float a = c.x - o0, bb = c.y - o1, cc = c.z - o2;
        const float d = __fmaf_rn(a, a, __fmaf_rn(bb, bb, cc * cc));
        if (d == b0) {
            if (seen == code) return j;
            ++seen;
        }
    }
    return -1;
}

// The two smallest exact float32 distances of a stream of candidates and the index of the smallest: the scan that
// decides where a key scan could not, or where there is none.
struct Top2 {
    const float o0, o1, o2;
    float b0 = kEdInf, b1 = kEdInf;
    int i0 = 0;
    __device__ __forceinline__ Top2(const float p0, const float p1, const float p2) : o0(p0), o1(p1), o2(p2) {}
    // candidate j with record c; !ok: a padding position of a list, read but not counted
    __device__ __forceinline__ void visit(const float4 c, const int j, const bool ok = true)
    {
        float d = ed_dist(c, o0, o1, o2);
        d = ok ? d : kEdInf;
        const bool lt0 = d < b0;
        b1 = lt0 ? b0 : (d < b1 ? d : b1);
        i0 = lt0 ? j : i0;
        b0 = lt0 ? d : b0;
    }
    // A gap of 2e-6 (relative) between the two smallest float32 distances proves the float64 order.  A RELATIVE margin only
    // (the variable-weight diffusers do not clamp their values, distances can be tiny -- and need no absolute margin: each
    // difference c - o is rounded once and the three squares are summed without cancellation, so the float32 distance is
    // within a few 2^-24 of the exact one however small it is; tests/test_gpu_steered_queries.py asks near ties down to 1e-7
    // of d0 and exact ties at fractional points, inside and beyond the cube).
    __device__ __forceinline__ bool decided() const { return b1 > b0 * 1.000002f; }
    // The answer: i0 when decided, else the tabulated choice at exact integer ties, else the float64 scan.
    // `cand`: all pal.K records.
    template <int CAP>
    __device__ __forceinline__ int finish(const PalDev &pal, const float4 *__restrict__ cand) const
    {
        if (decided()) return i0;
        if (b0 == b1) {
            const int tied = integer_tie_choice(pal, cand, o0, o1, o2, b0, i0);
            if (tied >= 0) return tied;
        }
        return nearest_f64<CAP>(pal, o0, o1, o2);
    }
};

// The whole palette, any point.
// `cand`: the palette as {x, y, z, out_rgb bits} -- in LDS for the wavefront kernels (every lane reads the same entry: one
// broadcast ds_read_b128 per colour, issued four at a time), in global memory for the serial ones.
template <int CAP>
__device__ __forceinline__ int nearest_color(const PalDev &pal, const float4 *__restrict__ cand, const float o0,
                                             const float o1, const float o2)
{
    Top2 t(o0, o1, o2);
    const int K = pal.K;
    int j = 0;
    for (; j + 4 <= K; j += 4) {
        const float4 c0 = cand[j], c1 = cand[j + 1], c2 = cand[j + 2], c3 = cand[j + 3];
        t.visit(c0, j);
        t.visit(c1, j + 1);
        t.visit(c2, j + 2);
        t.visit(c3, j + 3);
    }
    for (; j < K; ++j) t.visit(cand[j], j);
    return t.finish<CAP>(pal, cand);
}

// Index of a point's 16-wide cell in a 16x16x16 table: a point of the cube, and any point by its clamped coordinates (the
// extended tables, whose outermost cells stand for the half-spaces beyond the cube).
__device__ __forceinline__ uint32_t ed_cell16(const float o0, const float o1, const float o2)
{
    return ((uint32_t)o0 >> 4) | (((uint32_t)o1 >> 4) << 4) | (((uint32_t)o2 >> 4) << 8);
}
__device__ __forceinline__ uint32_t ed_cell16_clamped(const float o0, const float o1, const float o2)
{
    const int c0 = min(max((int)o0 >> 4, 0), 15), c1 = min(max((int)o1 >> 4, 0), 15), c2 = min(max((int)o2 >> 4, 0), 15);
    return (uint32_t)(c0 | (c1 << 4) | (c2 << 8));
}

// The scans below take their records through a plain pointer on purpose: inlined into a caller whose own pointer is
// __restrict__, a second __restrict__ here made the compiler split the third and fourth record read of a group into
// ds_read_b96 + ds_read_b32 in spite of keep_record_whole (seen in the assembly of ed_wavefront_kernel).

// ---- nibble lists (palettes of up to 16 colours): one word `e` per 16^3 cell, the count n in the low nibble (15: more
// than 7 entries, no list) and up to 7 palette indices in the nibbles above.  Unused positions hold an entry that is NOT on
// the list (ediff.hip, build_ed_cells), so the key scan evaluates whole groups without per-position tests.

// Key scan of a list of n <= 7: the entry, or -1 on a near tie.  8 instructions per position instead of the 16 of the
// exact scan.  `recs`: what the keys are made from -- the candidate records, decided at 3e-6 (relative), or (EXPANDED)
// their expanded records, decided at kEdExpandedMargin (absolute: see ed_key_expanded).
template <bool EXPANDED>
__device__ __forceinline__ int ed_nibble_key_scan(const uint32_t e, const int n, const float4 *recs, const float o0,
                                                  const float o1, const float o2)
{
    auto key = [&](const float4 r, const uint32_t tag) {
        return EXPANDED ? ed_key_expanded(r, o0, o1, o2, tag) : ed_key<3>(r, o0, o1, o2, tag);
    };
    const float4 r1 = recs[(e >> 4) & 15], r2 = recs[(e >> 8) & 15], r3 = recs[(e >> 12) & 15], r4 = recs[(e >> 16) & 15];
    KeyTop2 t;
    t.first3(key(r1, 1u), key(r2, 2u), key(r3, 3u));
    t.add(key(r4, 4u));
    if (n > 4) {
        const float4 r5 = recs[(e >> 20) & 15], r6 = recs[(e >> 24) & 15], r7 = recs[(e >> 28) & 15];
        t.add(key(r5, 5u));
        t.add(key(r6, 6u));
        t.add(key(r7, 7u));
    }
    bool decided;
    if (EXPANDED) decided = __int_as_float(t.m1 & ~7) - __int_as_float(t.m0 & ~7) > kEdExpandedMargin;
    else decided = t.decided<3>(1.000003f);
    return decided ? (int)((e >> (4 * (t.m0 & 7))) & 15u) : -1;
}

// Exact scan of the same list: four, then (n > 4) three records in flight together
__device__ __forceinline__ void ed_nibble_exact_scan(Top2 &t, const uint32_t e, const int n, const float4 *cand)
{
    const int j1 = (e >> 4) & 15, j2 = (e >> 8) & 15, j3 = (e >> 12) & 15, j4 = (e >> 16) & 15;
    const float4 c1 = cand[j1], c2 = cand[j2], c3 = cand[j3], c4 = cand[j4];
    t.visit(c1, j1, n >= 1);
    t.visit(c2, j2, n >= 2);
    t.visit(c3, j3, n >= 3);
    t.visit(c4, j4, n >= 4);
    if (n > 4) {
        const int j5 = (e >> 20) & 15, j6 = (e >> 24) & 15, j7 = (e >> 28) & 15;
        const float4 c5 = cand[j5], c6 = cand[j6], c7 = cand[j7];
        t.visit(c5, j5);
        t.visit(c6, j6, n >= 6);
        t.visit(c7, j7, n >= 7);
    }
}

// ---- byte lists (17..256 colours): a block of 16 bytes per cell, the count n in byte 0 -- 1..15 entries in bytes 1..n;
// 254: a crowded cell, refined (node number from bit 8 on); 255: no list.  The builder (ed_tables.h: pack)
// pads lists of up to 12 entries to a multiple of four positions with an entry that is not on the list; other unused bytes
// hold 0: a valid, ignored read.

__device__ __forceinline__ uint4 ed_drop_count_byte(uint4 blk)
{
    blk.x = __funnelshift_r(blk.x, blk.y, 8);
    blk.y = __funnelshift_r(blk.y, blk.z, 8);
    blk.z = __funnelshift_r(blk.z, blk.w, 8);
    blk.w >>= 8;
    return blk;
}

// Key scan of a list of 1 <= n <= 12 in groups of four, 4-bit tags: the entry, or -1 on a near tie
__device__ __forceinline__ int ed_byte_key_scan(const uint4 blk, const int n, const float4 *cand, const float o0,
                                                const float o1, const float o2)
{
    uint4 b = ed_drop_count_byte(blk);
    KeyTop2 t;
    uint32_t tag = 0u;
    for (int left = n; left > 0; left -= 4, tag += 4u) {
        const float4 c1 = cand[b.x & 255u], c2 = cand[(b.x >> 8) & 255u], c3 = cand[(b.x >> 16) & 255u], c4 = cand[b.x >> 24];
        t.add(ed_key<4>(c1, o0, o1, o2, tag));
        t.add(ed_key<4>(c2, o0, o1, o2, tag + 1u));
        t.add(ed_key<4>(c3, o0, o1, o2, tag + 2u));
        t.add(ed_key<4>(c4, o0, o1, o2, tag + 3u));
        b.x = b.y;
        b.y = b.z;
        b.z = 0u;
    }
    if (!t.decided<4>(1.000004f)) return -1;
    const uint32_t pos = ((uint32_t)t.m0 & 15u) + 1u;  // byte 1..12 of the block
    const uint32_t wsel = pos < 4u ? blk.x : (pos < 8u ? blk.y : (pos < 12u ? blk.z : blk.w));
    return (int)((wsel >> ((pos & 3u) * 8u)) & 255u);
}

// Exact scan of a list of 1 <= n <= 15: four entries per round, their reads in flight together
__device__ __forceinline__ void ed_byte_exact_scan(Top2 &t, const uint4 blk, int n, const float4 *cand)
{
    uint4 b = ed_drop_count_byte(blk);
    for (; n > 0; n -= 4) {
        const int j1 = (int)(b.x & 255u), j2 = (int)((b.x >> 8) & 255u), j3 = (int)((b.x >> 16) & 255u), j4 = (int)(b.x >> 24);
        const float4 c1 = cand[j1], c2 = cand[j2], c3 = cand[j3], c4 = cand[j4];
        t.visit(c1, j1);
        t.visit(c2, j2, n >= 2);
        t.visit(c3, j3, n >= 3);
        t.visit(c4, j4, n >= 4);
        b.x = b.y;
        b.y = b.z;
        b.z = b.w;
        b.w = 0u;
    }
}

// ---- wide lists (257..1024 colours): the same block with up to twelve ten-bit entries from bit 8 on, padded like the byte
// lists (ed_tables.h: ed_list_put; ediff.hip: ed_cells_kernel)

// entry `pos` (0-based) of a wide block
__device__ __forceinline__ int ed_wide_entry(const uint4 blk, const uint32_t pos)
{
    const uint32_t off = 8u + 10u * pos, wi = off >> 5, sh = off & 31u;
    const uint32_t lo = wi == 0u ? blk.x : (wi == 1u ? blk.y : (wi == 2u ? blk.z : blk.w));
    const uint32_t hi = wi == 0u ? blk.y : (wi == 1u ? blk.z : (wi == 2u ? blk.w : 0u));
    return (int)(__funnelshift_r(lo, hi, sh) & 1023u);
}

// Key scan of a list of n <= 12 in groups of four, 4-bit tags: the entry, or -1 on a near tie or an empty list
__device__ __forceinline__ int ed_wide_key_scan(const uint4 blk, const int n, const float4 *cand, const float o0,
                                                const float o1, const float o2)
{
    KeyTop2 t;
    for (uint32_t g = 0; (int)g < n; g += 4u) {
        const float4 c1 = cand[ed_wide_entry(blk, g)], c2 = cand[ed_wide_entry(blk, g + 1u)], c3 = cand[ed_wide_entry(blk, g + 2u)],
                     c4 = cand[ed_wide_entry(blk, g + 3u)];
        t.add(ed_key<4>(c1, o0, o1, o2, g));
        t.add(ed_key<4>(c2, o0, o1, o2, g + 1u));
        t.add(ed_key<4>(c3, o0, o1, o2, g + 2u));
        t.add(ed_key<4>(c4, o0, o1, o2, g + 3u));
    }
    return n >= 1 && t.decided<4>(1.000004f) ? ed_wide_entry(blk, (uint32_t)t.m0 & 15u) : -1;
}

// Exact scan of the n listed entries
__device__ __forceinline__ void ed_wide_exact_scan(Top2 &t, const uint4 blk, const int n, const float4 *cand)
{
    for (int i = 0; i < n; ++i) {
        const int j = ed_wide_entry(blk, (uint32_t)i);
        t.visit(cand[j], j);
    }
}

// ---- the hierarchical table of at most four entries per leaf (ed_tables.h: ed_build_h4; palettes of 17..256 colours).
// The wave pays for the longest candidate list among its 64 lanes, so instead of scanning a 16^3 cell's list in rounds of
// four, a lane whose cell has more than four possible nearest entries descends to the cell's 8-wide child and, if need be, to
// the 4-wide and 2-wide ones -- at most three more dependent reads -- and ranks ONE group of four.
// `h4`: words [0, 4096) the 16^3 cells, then eight words per node; a word is a leaf's four palette indices, or a marker
// (byte 0 >= byte 1) with the node number in its high half (0xffff: no answer below).  `cand`: the palette's records.  A
// point of the cube only.  Returns the palette index, or -1 when the table has no answer for this point (a 2-wide cell that
// is still longer, or a float32 near tie): the caller's lists decide then.
__device__ __forceinline__ bool h4_marker(const uint32_t w) { return (w & 0xffu) >= ((w >> 8) & 0xffu); }

__device__ __forceinline__ int nearest_h4(const uint32_t *__restrict__ h4, const float4 *__restrict__ cand, const float o0, const float o1,
                                          const float o2)
{
    const uint32_t i0 = (uint32_t)o0, i1 = (uint32_t)o1, i2 = (uint32_t)o2;
    uint32_t w = h4[ed_cell16(o0, o1, o2)];
#pragma unroll
    for (int bit = 3; bit >= 1; --bit) {   // the 8-wide, 4-wide, 2-wide child: as far as this lane's cell is cut
        if (!h4_marker(w)) break;
        if ((w >> 16) == 0xffffu) return -1;
        w = h4[4096u + (w >> 16) * 8u + (((i0 >> bit) & 1u) | (((i1 >> bit) & 1u) << 1) | (((i2 >> bit) & 1u) << 2))];
    }
    if (h4_marker(w)) return -1;
    const float4 c1 = cand[w & 255u], c2 = cand[(w >> 8) & 255u], c3 = cand[(w >> 16) & 255u], c4 = cand[w >> 24];
    keep_record_whole(c1);
    keep_record_whole(c2);
    keep_record_whole(c3);
    keep_record_whole(c4);
    KeyTop2 t;
    t.first3(ed_key<3>(c1, o0, o1, o2, 0u), ed_key<3>(c2, o0, o1, o2, 1u), ed_key<3>(c3, o0, o1, o2, 2u));
    t.add(ed_key<3>(c4, o0, o1, o2, 3u));
    return t.decided<3>(1.000003f) ? (int)((w >> (8u * ((uint32_t)t.m0 & 3u))) & 255u) : -1;
}

// nearest_color for a point of the cube, restricted to the candidate list of the point's cell (same validation, same
// fallbacks).  The tables, tried in this order; all but pal.ed_cells are optional (nullptr: not there):
//   `coarse` + `expanded`  palettes of up to 16 colours, wavefront kernels: an LDS copy of the nibble lists of the 16^3 cells
//              -- 99.8 % of the cells of a 16-colour palette have at most 7 entries; a step then needs no load from global
//              memory at all (the 8^3 lists live in L2: ~600 cycles of latency that every step of the dependency chain would
//              pay).  EXPANDED instances rank by `expanded`, the candidates' expanded records (ed_key_expanded), first.
//   `h4`       17..256 colours: the hierarchical table (nearest_h4).
//   `lists16`  17..256 colours, wavefront kernel on the few-frames schedule: an LDS copy of the byte lists of the 16^3 cells
//              (count 255: more than 15 entries, use the 8^3 table).
//   pal.ed_cells, pal.ed_nodes  the byte (or wide) lists of the 8x8x8 cells in global memory and the octree below the
//              crowded ones (4^3, 2^3, 1^3 sub-cells).
// `cand`: all pal.K records.  A list longer than 15 entries sends the point through the whole palette.
// WIDE_OK: the instance also reads the wide blocks of palettes above 256 colours (only the large-queue instances do: the
// launchers send every such palette there).
template <int CAP, bool EXPANDED = false, bool WIDE_OK = false>
__device__ __forceinline__ int nearest_color_cells(const PalDev &pal, const float4 *__restrict__ cand,
                                                   const uint32_t *__restrict__ coarse, const float o0, const float o1,
                                                   const float o2, const uint4 *__restrict__ lists16 = nullptr,
                                                   const float4 *__restrict__ expanded = nullptr, const uint32_t *__restrict__ h4 = nullptr)
{
    Top2 t(o0, o1, o2);
    bool listed = false;
    if (coarse) {
        const uint32_t e = coarse[ed_cell16(o0, o1, o2)];
        const int n = (int)(e & 15u);
        if (n <= 7) {
            const int j = ed_nibble_key_scan<EXPANDED>(e, n, EXPANDED ? expanded : cand, o0, o1, o2);
            if (j >= 0) return j;
            ed_nibble_exact_scan(t, e, n, cand);
            listed = true;
        }
    }
    if (!listed && h4) {
        const int j = nearest_h4(h4, cand, o0, o1, o2);
        if (j >= 0) return j;
    }
    if (!listed) {
        uint4 blk = make_uint4(255u, 0u, 0u, 0u);
        if (lists16) blk = lists16[ed_cell16(o0, o1, o2)];
        int n = (int)(blk.x & 255u);
        if (n == 255) {  // (no LDS lists, or a cell with more than 15 entries)
            const uint32_t ci = ((uint32_t)o0 >> 3) | (((uint32_t)o1 >> 3) << 5) | (((uint32_t)o2 >> 3) << 10);
            blk = pal.ed_cells[ci];
            n = (int)(blk.x & 255u);
        }
        if (n == 254) {  // a crowded cell (clustered palettes): refined into 4^3, 2^3, 1^3 sub-cells
            const uint32_t i0 = (uint32_t)o0, i1 = (uint32_t)o1, i2 = (uint32_t)o2;
            for (int bit = 2; n == 254; --bit) {
                const uint32_t sub = ((i0 >> bit) & 1u) | (((i1 >> bit) & 1u) << 1) | (((i2 >> bit) & 1u) << 2);
                blk = pal.ed_nodes[(size_t)(blk.x >> 8) * 8 + sub];
                n = (int)(blk.x & 255u);
            }
        }
        if (n > 15) return nearest_color<CAP>(pal, cand, o0, o1, o2);
        if (WIDE_OK && pal.K > 256) {
            const int j = ed_wide_key_scan(blk, n, cand, o0, o1, o2);
            if (j >= 0) return j;
            ed_wide_exact_scan(t, blk, n, cand);
        } else {
            if (n >= 1 && n <= 12 && pal.K > 16) {
                const int j = ed_byte_key_scan(blk, n, cand, o0, o1, o2);
                if (j >= 0) return j;
            }
            ed_byte_exact_scan(t, blk, n, cand);
        }
    }
    return t.finish<CAP>(pal, cand);
}

// Palettes of up to 16 colours, any query point: the nibble-list key scan over the list of the point's cell in the EXTENDED
// 16^3 table `ext` (ediff.hip, build_ed_cells: the outermost cells stand for the half-spaces beyond the cube, a point is
// looked up by its clamped coordinates).  `cand`: all pal.K records.  The variable-weight diffusers do not clamp their
// values, and a wave nearly always holds a point outside the cube: without this every step scanned the whole palette.
template <int CAP>
__device__ __forceinline__ int nearest_ext(const PalDev &pal, const float4 *__restrict__ cand, const uint32_t *__restrict__ ext,
                                           const float o0, const float o1, const float o2)
{
    const uint32_t e = ext[ed_cell16_clamped(o0, o1, o2)];
    const int n = (int)(e & 15u);
    if (n <= 7) {
        const int j = ed_nibble_key_scan<false>(e, n, cand, o0, o1, o2);
        if (j >= 0) return j;
    }
    return nearest_color<CAP>(pal, cand, o0, o1, o2);  // long lists, near ties, exact ties: the full scan and its validation
}

// Palettes of 17..1024 colours, any query point: the key scan over the byte (above 256 colours: wide) list of the point's
// cell in the extended 16^3 table `ext16` (ed_tables.h: ed_build_ext16 -- the outermost cells are unbounded, a point is
// looked up by its clamped coordinates) and the octree pal.ed_ext_nodes below its crowded outermost cells.  `cand`: all
// pal.K records, in LDS; `inside`: the point lies in the cube, where pal.ed_cells (if there) has lists for the cells whose
// extended list is too long.  Near ties of a list go to its exact scan, what that cannot decide and exact ties to the full
// scan and its validation.  Call it in wave-uniform control flow: the __ballot below decides for the wave.
template <int CAP>
__device__ __forceinline__ int nearest_ext16(const PalDev &pal, const float4 *__restrict__ cand, const uint4 *__restrict__ ext16,
                                             const float o0, const float o1, const float o2, const bool inside)
{
    uint4 blk = ext16[ed_cell16_clamped(o0, o1, o2)];
    int n = (int)(blk.x & 255u);
    if (n == 254) {
        // an outermost cell with too long a list: down its octree by the CLAMPED integer coordinates (a point beyond the cube falls
        // into the outer children, which are unbounded on that side); sizes 8, 4, 2, 1 -- a unit child is a list or 255
        const uint32_t i0 = (uint32_t)min(max((int)o0, 0), 255), i1 = (uint32_t)min(max((int)o1, 0), 255), i2 = (uint32_t)min(max((int)o2, 0), 255);
        for (int bit = 3; n == 254 && bit >= 0; --bit) {
            const uint32_t sub = ((i0 >> bit) & 1u) | (((i1 >> bit) & 1u) << 1) | (((i2 >> bit) & 1u) << 2);
            blk = pal.ed_ext_nodes[(size_t)(blk.x >> 8) * 8 + sub];
            n = (int)(blk.x & 255u);
        }
    }
    // A lane whose cell has no usable list and whose point lies beyond the cube must scan the whole palette -- and then the wave
    // executes that scan anyway: all its lanes take it, instead of the scan PLUS the list paths of the others (a palette crowded at a
    // face of the cube -- any palette under use_gamma, at the dark end -- has such a lane in most waves: 256 colours 59 -> 87 ms per
    // 1080p frame with the three paths side by side).
    if (__ballot((n < 1 || n > 15) && !(inside && pal.ed_cells != nullptr)) != 0ull) return nearest_color<CAP>(pal, cand, o0, o1, o2);
    Top2 t(o0, o1, o2);
    if (pal.K > 256) {
        if (n >= 1 && n <= 12) {
            const int j = ed_wide_key_scan(blk, n, cand, o0, o1, o2);
            if (j >= 0) return j;
            ed_wide_exact_scan(t, blk, n, cand);
            if (t.decided()) return t.i0;
        }
        if (n > 12 && inside && pal.ed_cells) return nearest_color_cells<CAP, false, CAP == kQueueLarge>(pal, cand, nullptr, o0, o1, o2, nullptr, nullptr, nullptr);
        return nearest_color<CAP>(pal, cand, o0, o1, o2);
    }
    if (n >= 1 && n <= 12) {
        const int j = ed_byte_key_scan(blk, n, cand, o0, o1, o2);
        if (j >= 0) return j;
    }
    if (n >= 1 && n <= 15) {
        // longer lists and near ties of the key scan: the exact scan over the LISTED entries only (a wave pays for the slowest of
        // its 64 lanes: sending it through the whole palette for one lane's 13-entry list cost most of the gain)
        ed_byte_exact_scan(t, blk, n, cand);
        if (t.decided()) return t.i0;
    }
    // a 16-wide cell with more than 15 possible nearest entries (a crowded palette -- e.g. any palette under use_gamma, whose dark
    // entries crowd the low end of the linear scale): a point INSIDE the cube has the 8^3 lists and their octree (error diffusion's
    // path); only points beyond the cube in such a cell scan the whole palette
    if (n > 15 && inside && pal.ed_cells) return nearest_color_cells<CAP, false, false>(pal, cand, nullptr, o0, o1, o2, nullptr, nullptr, nullptr);
    return nearest_color<CAP>(pal, cand, o0, o1, o2);
}

// ---- the one-wave-per-frame kernels: one point per step, the palette spread over the lanes, entry l + 64 m in pc[m] of
// lane l (records past the palette hold 1e30: their distance overflows to +inf).  Callers: os_rowserial_kernel and
// riemersma_kernel; ed_rowserial_kernel (ediff.hip) has the same scan open-coded, see the head of this file.

struct WaveNearest {
    int j;          // the entry with the smallest float32 distance (the lowest lane's, among equal ones)
    int winner;     // the lane that holds it
    bool near_tie;  // another entry lies within the margin of Top2::decided: j is not proven
};

// Must be called by all 64 lanes in uniform control flow, with the same point in every lane: it reduces with DPP, votes
// with __ballot and reads with v_readlane; the result is the same in every lane (scalar registers).
// The second smallest distance is only needed for the margin test "b1 > b0 * 1.000002": it fails iff some other entry lies
// within the margin, i.e. more than one lane passes, or a lane's own runner-up does.
template <int M>
__device__ __forceinline__ WaveNearest wave_nearest(const float4 (&pc)[M], const int lane, const float o0, const float o1, const float o2)
{
    float b0 = kEdInf, b1 = kEdInf;
    int i0 = lane;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float da = pc[m].x - o0, db = pc[m].y - o1, dc = pc[m].z - o2;
        const float d = __fmaf_rn(da, da, __fmaf_rn(db, db, dc * dc));
        const bool lt0 = d < b0;
        b1 = lt0 ? b0 : (d < b1 ? d : b1);
        i0 = lt0 ? lane + 64 * m : i0;
        b0 = lt0 ? d : b0;
    }
    const float B0 = wave_min_to_all(b0);
    const unsigned long long wm = __ballot(b0 == B0);
    WaveNearest r;
    r.winner = __ffsll((long long)wm) - 1;
    const float lim = B0 * 1.000002f;
    const unsigned long long close = __ballot(b0 <= lim);
    r.near_tie = (close & (close - 1ull)) != 0ull || (M > 1 && __ballot(b1 <= lim) != 0ull);
    r.j = M == 1 ? r.winner : __builtin_amdgcn_readlane(i0, r.winner);
    return r;
}

// The record of the step's answer, {x, y, z, out_rgb bits}: the winner's by v_readlane (M == 1) or one LDS broadcast read
// (`s_pal`: all pal.K records, in LDS; used when M > 1 only); on a near tie that of nearest_f64's entry, from pal.fcand.
// Uniform control flow, as wave_nearest.  The LDS read names its address space: behind a plain pointer the compiler merged
// it with the read from pal.fcand into one flat_load of a selected address (2 % on a 256-colour step of these kernels).
typedef float ed_float4_t __attribute__((ext_vector_type(4)));
template <int CAP, int M>
__device__ __forceinline__ float4 wave_nearest_record(const PalDev &pal, const float4 (&pc)[M], const float4 *__restrict__ s_pal,
                                                      const WaveNearest r, const float o0, const float o1, const float o2)
{
    float cx, cy, cz, cw;
    if (!r.near_tie) {
        if (M == 1) {
            cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pc[0].x), r.winner));
            cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pc[0].y), r.winner));
            cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pc[0].z), r.winner));
            cw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pc[0].w), r.winner));
        } else {
            const ed_float4_t c = *(const __attribute__((address_space(3))) ed_float4_t *)(s_pal + r.j);
            cx = c.x;
            cy = c.y;
            cz = c.z;
            cw = c.w;
        }
    } else {  // near tie: float64 scan, scipy's traversal on exact ties
        const float4 c = pal.fcand[nearest_f64<CAP>(pal, o0, o1, o2)];
        cx = c.x;
        cy = c.y;
        cz = c.z;
        cw = c.w;
    }
    return make_float4(cx, cy, cz, cw);
}

}  // namespace
}  // namespace dp
