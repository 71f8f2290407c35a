// Halftone dithering (HalftoneDitherStrategy.dither, dithering_lib.py:1498-1695): a rotated screen of cells, each cell's
// mean colour mapped to its nearest palette entry, a pixel inked with its cell's entry when its darkness exceeds the
// screen threshold.
//
// Per group of frames (the cells of every frame in the workspace at once):
//   ht_cell_kernel    64 x 16 pixel tiles: each pixel's channel values and a count go into its cell's four uint32 words.
//                     The cells a tile touches form a small rectangle of cell coordinates (the four corners bound it:
//                     each rotated coordinate is monotone in x and in y), summed in LDS first; one global atomic per
//                     occupied cell and word then.  Integer sums are exact in any order, as the reference's float64
//                     bincount of integers is.
//   ht_colour_kernel  per occupied cell: mean = sum / count in float64, nearest entry by a float64 scan; exact ties go
//                     to a list for ht_tie_kernel (scipy's traversal replay, a small grid: its queue lives in scratch).
//   ht_ink_kernel     per pixel: the float64 threshold chain, float32 darkness, the cell's colour or the paper colour.
// The screen is recomputed in every pass that needs it, not cached per geometry.  That ~40 float64 operations per pixel
// cost less than reading a cached float32 + int32 back from HBM is an assumption: a cached variant was not built or measured.
//
// Grid bounds: the host derives cx_min, cy_min, max_x, max_y from the four image corners with the same IEEE operations the
// kernels use (no contraction, correctly rounded division), and each rotated coordinate is monotone in x and in y, so every
// pixel's cell lies inside the grid and inside its tile's corner rectangle.  The range checks below can therefore not fail;
// they only keep a store inside the workspace should that reasoning ever break (a pixel outside its tile's rectangle still
// goes to the global sums; one outside the grid would be left out, or inked with the paper colour).
#include <cmath>

#include "dp_internal.h"
#include "tree_query.hip.h"

namespace dp {
namespace {

constexpr int kTileW = 64, kTileH = 16, kBlock = 256;
constexpr int kWinCells = 2048;              // LDS cells per tile (32 KB); tiles that touch more add to HBM directly
constexpr int kPowUlps = 64;                 // the device pow is trusted to this many float64 ulps of numpy's
constexpr size_t kGroupBytes = 256u << 20;   // cells of the frames that run at once
constexpr size_t kHeadBytes = 256;           // workspace head: the exact-tie count

struct HtGeom {
    double cs, c, s, e, mn, span, sharp;
    int cls, shape, sharpen;
    int cx_min, cy_min, max_x, max_y;
    int h, w;
    int paper;  // paper_idx
    const int32_t *fix_idx;
    const float *fix_thr;
    int64_t n_fix;
};

// x_rot, y_rot (dithering_lib.py:1664-1665): each product rounded, then the sum
__device__ __forceinline__ void ht_rot(const HtGeom &g, const int x, const int y, double &xr, double &yr)
{
    const double X = (double)x, Y = (double)y;
    xr = __dsub_rn(__dmul_rn(X, g.c), __dmul_rn(Y, g.s));
    yr = __dadd_rn(__dmul_rn(X, g.s), __dmul_rn(Y, g.c));
}

// np.floor(r / cell_size).astype(np.int32) (:1667-1668)
__device__ __forceinline__ int ht_cell_coord(const double r, const double cs) { return (int)floor(__ddiv_rn(r, cs)); }

// numpy's float remainder (npy_divmod): fmod, plus the divisor when the signs differ; +0 for an exact multiple
__device__ __forceinline__ double np_mod(const double a, const double b)
{
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m = __dadd_rn(m, b);
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// np.clip(t, 0.0, 1.0): minimum(maximum(t, 0), 1)
__device__ __forceinline__ double ht_clip01(double t)
{
    t = t > 0.0 ? t : 0.0;
    return t < 1.0 ? t : 1.0;
}

// the chain after the exponent (:1688-1693)
__device__ __forceinline__ float ht_finish(const HtGeom &g, const double p)
{
    double t = __dadd_rn(g.mn, __dmul_rn(p, g.span));
    if (g.sharpen) t = __dadd_rn(0.5, __dmul_rn(__dsub_rn(t, 0.5), g.sharp));
    return __double2float_rn(ht_clip01(t));
}

// float32 screen threshold at rotated position (xr, yr); amb: the pow class could not decide it (see dp_halftone_pow_flags)
__device__ __forceinline__ float ht_threshold(const HtGeom &g, const double xr, const double yr, bool &amb)
{
    amb = false;
    const double dx = __dsub_rn(__ddiv_rn(np_mod(xr, g.cs), g.cs), 0.5);
    const double dy = __dsub_rn(__ddiv_rn(np_mod(yr, g.cs), g.cs), 0.5);
    double dist, max_dist;
    if (g.shape == DP_HT_SHAPE_SQUARE) {
        const double ax = fabs(dx), ay = fabs(dy);
        dist = ax > ay ? ax : ay;
        max_dist = 0.5;
    } else if (g.shape == DP_HT_SHAPE_DIAMOND) {
        dist = __dadd_rn(fabs(dx), fabs(dy));
        max_dist = 1.0;
    } else {
        dist = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        max_dist = 0.5;
    }
    const double dn = ht_clip01(__ddiv_rn(dist, max_dist));
    if (g.cls == DP_HT_EXP_IDENTITY) return ht_finish(g, dn);
    if (g.cls == DP_HT_EXP_SQRT) return ht_finish(g, __dsqrt_rn(dn));
    if (g.cls == DP_HT_EXP_SQUARE) return ht_finish(g, __dmul_rn(dn, dn));
    const double p = pow(dn, g.e);
    const float f = ht_finish(g, p);
    if (dn > 0.0 && dn < 1.0) {  // pow(0, e) and pow(1, e) are exact everywhere
        const long long b = __double_as_longlong(p);
        const double lo = __longlong_as_double(b > kPowUlps ? b - kPowUlps : 0ll);
        const double hi = __longlong_as_double(b + kPowUlps);
        amb = ht_finish(g, lo) != f || ht_finish(g, hi) != f;
    }
    return f;
}

__device__ __forceinline__ void ht_load(const uint8_t *__restrict__ px, const uint8_t *__restrict__ lut, uint32_t &r,
                                        uint32_t &gg, uint32_t &b)
{
    r = px[0];
    gg = px[1];
    b = px[2];
    if (lut) {
        r = lut[r];
        gg = lut[gg];
        b = lut[b];
    }
}

__global__ __launch_bounds__(kBlock) void ht_cell_kernel(const uint8_t *__restrict__ in, uint32_t *__restrict__ cells,
                                                         const HtGeom g, const uint8_t *__restrict__ lut, const int tiles_x,
                                                         const size_t S)
{
    __shared__ uint32_t s_win[kWinCells * 4];
    const int t = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTileW, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTileH;
    const int tx1 = min(tx0 + kTileW - 1, g.w - 1), ty1 = min(ty0 + kTileH - 1, g.h - 1);
    const size_t npx = (size_t)g.h * (size_t)g.w;
    const uint8_t *fin = in + (size_t)blockIdx.y * npx * 3;
    uint32_t *fc = cells + (size_t)blockIdx.y * S * 4;

    // the tile's rectangle of cell coordinates, from its corners
    int wx0 = INT32_MAX, wx1 = INT32_MIN, wy0 = INT32_MAX, wy1 = INT32_MIN;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double xr, yr;
        ht_rot(g, (k & 1) ? tx1 : tx0, (k & 2) ? ty1 : ty0, xr, yr);
        const int cx = ht_cell_coord(xr, g.cs), cy = ht_cell_coord(yr, g.cs);
        wx0 = min(wx0, cx);
        wx1 = max(wx1, cx);
        wy0 = min(wy0, cy);
        wy1 = max(wy1, cy);
    }
    const long long wxn = (long long)wx1 - wx0 + 1, wyn = (long long)wy1 - wy0 + 1;
    const bool use_lds = wxn * wyn <= kWinCells;
    const int nwin = use_lds ? (int)(wxn * wyn) : 0;
    for (int i = t; i < nwin * 4; i += kBlock) s_win[i] = 0u;
    __syncthreads();

    const int x = tx0 + (t & (kTileW - 1));
    for (int yy = ty0 + (t >> 6); yy <= ty1; yy += kBlock / kTileW) {
        if (x > tx1) break;
        uint32_t r, gg, b;
        ht_load(fin + ((size_t)yy * g.w + x) * 3, lut, r, gg, b);
        double xr, yr;
        ht_rot(g, x, yy, xr, yr);
        const int cx = ht_cell_coord(xr, g.cs), cy = ht_cell_coord(yr, g.cs);
        if (use_lds && cx >= wx0 && cx <= wx1 && cy >= wy0 && cy <= wy1) {   // (always, see "Grid bounds" above)
            const int wi = (cy - wy0) * (int)wxn + (cx - wx0);
            atomicAdd(&s_win[wi * 4 + 0], r);
            atomicAdd(&s_win[wi * 4 + 1], gg);
            atomicAdd(&s_win[wi * 4 + 2], b);
            atomicAdd(&s_win[wi * 4 + 3], 1u);
        } else {
            const int ox = cx - g.cx_min, oy = cy - g.cy_min;
            if ((unsigned)ox < (unsigned)g.max_x && (unsigned)oy < (unsigned)g.max_y) {   // (always: "Grid bounds")
                uint32_t *c = fc + ((size_t)oy * (size_t)g.max_x + (size_t)ox) * 4;
                atomicAdd(c + 0, r);
                atomicAdd(c + 1, gg);
                atomicAdd(c + 2, b);
                atomicAdd(c + 3, 1u);
            }
        }
    }
    if (!use_lds) return;
    __syncthreads();
    for (int i = t; i < nwin; i += kBlock) {
        const uint32_t n = s_win[i * 4 + 3];
        if (n == 0u) continue;
        const int ox = wx0 + i % (int)wxn - g.cx_min, oy = wy0 + i / (int)wxn - g.cy_min;
        if ((unsigned)ox < (unsigned)g.max_x && (unsigned)oy < (unsigned)g.max_y) {
            uint32_t *c = fc + ((size_t)oy * (size_t)g.max_x + (size_t)ox) * 4;
            atomicAdd(c + 0, s_win[i * 4 + 0]);
            atomicAdd(c + 1, s_win[i * 4 + 1]);
            atomicAdd(c + 2, s_win[i * 4 + 2]);
            atomicAdd(c + 3, n);
        }
    }
}

__device__ __forceinline__ void ht_mean(const uint4 v, const uint32_t n, double &m0, double &m1, double &m2)
{
    const double cnt = (double)n;  // np.maximum(count, 1): occupied cells only
    m0 = __ddiv_rn((double)v.x, cnt);
    m1 = __ddiv_rn((double)v.y, cnt);
    m2 = __ddiv_rn((double)v.z, cnt);
}

// Cell words after this pass: x = the output colour r | g<<8 | b<<16 of the nearest entry; an exact float64 tie (palettes
// of more than one KD-tree leaf) keeps the sums, sets bit 31 of the count and queues the cell for ht_tie_kernel.
__global__ __launch_bounds__(kBlock) void ht_colour_kernel(uint32_t *__restrict__ cells, const size_t S, const PalDev pal,
                                                           uint32_t *__restrict__ ties, uint32_t *__restrict__ n_ties)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= S) return;
    const size_t e = (size_t)blockIdx.y * S + i;
    uint4 *c = reinterpret_cast<uint4 *>(cells) + e;
    const uint4 v = *c;
    if (v.w == 0u) return;
    double m0, m1, m2;
    ht_mean(v, v.w, m0, m1, m2);
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double b0 = inf, b1 = inf;
    int i0 = 0;
    const int K = pal.K;
    for (int j = 0; j < K; ++j) {
        const double d = sq_dist3(pal.pts + 3 * j, m0, m1, m2);
        if (d < b0) {
            b1 = b0;
            b0 = d;
            i0 = j;
        } else if (d < b1) {
            b1 = d;
        }
    }
    if (b0 == b1 && K > kLeafSize) {
        ties[atomicAdd(n_ties, 1u)] = (uint32_t)e;
        reinterpret_cast<uint32_t *>(c)[3] = v.w | 0x80000000u;
    } else {
        reinterpret_cast<uint32_t *>(c)[0] = pal.out_rgb[i0];
    }
}

template <int CAP>
__global__ __launch_bounds__(64) void ht_tie_kernel(uint32_t *__restrict__ cells, const uint32_t *__restrict__ ties,
                                                    const uint32_t *__restrict__ n_ties, const PalDev pal)
{
    const uint32_t n = *n_ties;
    for (uint32_t k = blockIdx.x * 64u + threadIdx.x; k < n; k += gridDim.x * 64u) {
        uint4 *c = reinterpret_cast<uint4 *>(cells) + ties[k];
        const uint4 v = *c;
        double m0, m1, m2;
        ht_mean(v, v.w & 0x7fffffffu, m0, m1, m2);
        double d2[1];
        int ii[1];
        tree_query<1, CAP>(pal, m0, m1, m2, d2, ii);
        reinterpret_cast<uint32_t *>(c)[0] = pal.out_rgb[ii[0]];
    }
}

// the caller's threshold for a pixel the pow class could not decide (binary search of the ascending list)
__device__ __forceinline__ float ht_fixed(const HtGeom &g, const int32_t p, const float own)
{
    int64_t lo = 0, hi = g.n_fix;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (g.fix_idx[mid] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < g.n_fix && g.fix_idx[lo] == p) ? g.fix_thr[lo] : own;
}

__global__ __launch_bounds__(kBlock) void ht_ink_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                        const uint32_t *__restrict__ cells, const HtGeom g,
                                                        const uint8_t *__restrict__ lut, const uint32_t *__restrict__ out_rgb,
                                                        const size_t S)
{
    const size_t npx = (size_t)g.h * (size_t)g.w;
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / (unsigned)g.w), x = (int)(p - (size_t)y * (unsigned)g.w);
    const size_t off = ((size_t)blockIdx.y * npx + p) * 3;
    uint32_t r, gg, b;
    ht_load(in + off, lut, r, gg, b);
    // gray = 0.299 R + 0.587 G + 0.114 B in float32 (the Python constants become float32 under NEP 50), / 255, 1 - gray
    const float c0 = __int_as_float(0x3e991687), c1 = __int_as_float(0x3f1645a2), c2 = __int_as_float(0x3de978d5);
    const float gray = __fadd_rn(__fadd_rn(__fmul_rn(c0, (float)r), __fmul_rn(c1, (float)gg)), __fmul_rn(c2, (float)b));
    const float dark = __fsub_rn(1.0f, __fdiv_rn(gray, 255.0f));
    double xr, yr;
    ht_rot(g, x, y, xr, yr);
    bool amb;
    float thr = ht_threshold(g, xr, yr, amb);
    if (amb && g.n_fix > 0) thr = ht_fixed(g, (int32_t)p, thr);
    uint32_t col = out_rgb[g.paper];
    if (dark > thr) {
        const int ox = ht_cell_coord(xr, g.cs) - g.cx_min, oy = ht_cell_coord(yr, g.cs) - g.cy_min;
        if ((unsigned)ox < (unsigned)g.max_x && (unsigned)oy < (unsigned)g.max_y)   // (always: "Grid bounds")
            col = cells[((size_t)blockIdx.y * S + (size_t)oy * (size_t)g.max_x + (size_t)ox) * 4];
    }
    uint8_t *o = out + off;
    o[0] = (uint8_t)col;
    o[1] = (uint8_t)(col >> 8);
    o[2] = (uint8_t)(col >> 16);
}

__global__ __launch_bounds__(kBlock) void ht_flags_kernel(const HtGeom g, int32_t *__restrict__ idx, const int64_t cap,
                                                          unsigned long long *__restrict__ count)
{
    const size_t npx = (size_t)g.h * (size_t)g.w;
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / (unsigned)g.w), x = (int)(p - (size_t)y * (unsigned)g.w);
    double xr, yr;
    ht_rot(g, x, y, xr, yr);
    bool amb;
    (void)ht_threshold(g, xr, yr, amb);
    if (amb) {
        const unsigned long long k = atomicAdd(count, 1ull);
        if (k < (unsigned long long)cap) idx[k] = (int32_t)p;
    }
}

// host: the same rotation and division as the kernels (IEEE float64, no contraction)
void corner_cell(const dp_halftone_params &P, const int x, const int y, double &cx, double &cy)
{
    const double X = (double)x, Y = (double)y;
    const double xr = X * P.cos_a - Y * P.sin_a;
    const double yr = X * P.sin_a + Y * P.cos_a;
    cx = std::floor(xr / P.cell_size);
    cy = std::floor(yr / P.cell_size);
}

}  // namespace

// The cell grid of an h x w frame (dithering_lib.py:1667-1673): minima and extents from the four corners.  DP_OK, or
// DP_EUNSUPPORTED (with the error text) for grids the reference's int32 ids or the uint32 sums cannot hold.
static int halftone_grid(int h, int w, const dp_halftone_params &P, int &cx_min, int &cy_min, int &max_x, int &max_y,
                         size_t &S)
{
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int k = 0; k < 4; ++k) {
        double cx, cy;
        corner_cell(P, (k & 1) ? w - 1 : 0, (k & 2) ? h - 1 : 0, cx, cy);
        x0 = std::fmin(x0, cx);
        x1 = std::fmax(x1, cx);
        y0 = std::fmin(y0, cy);
        y1 = std::fmax(y1, cy);
    }
    const double lim = 2147483647.0;
    if (!(x0 >= -lim - 1 && x1 <= lim && y0 >= -lim - 1 && y1 <= lim)) {
        set_error("dp_halftone_u8: cell coordinates outside int32 (cell_size too small for the image)");
        return DP_EUNSUPPORTED;
    }
    const double nx = x1 - x0 + 1.0, ny = y1 - y0 + 1.0;
    if (nx * ny > lim) {
        set_error("dp_halftone_u8: more than 2^31 - 1 cells (cell_size too small for the image)");
        return DP_EUNSUPPORTED;
    }
    // uint32 channel sums: a cell holds at most (ceil(cell_size) + 2)^2 pixels, and never more than the image
    const double side = std::ceil(P.cell_size) + 2.0;
    const double most = std::fmin(side * side, (double)h * (double)w);
    if (most * 255.0 > 4294967295.0) {
        set_error("dp_halftone_u8: cells of more than 16843009 pixels are not supported");
        return DP_EUNSUPPORTED;
    }
    cx_min = (int)x0;
    cy_min = (int)y0;
    max_x = (int)nx;
    max_y = (int)ny;
    S = (size_t)max_x * (size_t)max_y;
    return DP_OK;
}

static int64_t halftone_group(int64_t n_frames, size_t S)
{
    const size_t per = S * 20;  // 16 bytes of cell words + one tie-list word per cell
    int64_t g = (int64_t)(kGroupBytes / (per ? per : 1));
    if (g < 1) g = 1;
    if (g > 65535) g = 65535;
    return g < n_frames ? g : n_frames;
}

size_t halftone_ws_bytes(int64_t n_frames, int h, int w, const dp_halftone_params &P)
{
    int cx_min, cy_min, max_x, max_y;
    size_t S;
    if (n_frames <= 0 || h <= 0 || w <= 0) return 0;
    if (halftone_grid(h, w, P, cx_min, cy_min, max_x, max_y, S) != DP_OK) return 0;
    return kHeadBytes + (size_t)halftone_group(n_frames, S) * S * 20;
}

static HtGeom make_geom(int h, int w, const dp_halftone_params &P, int cx_min, int cy_min, int max_x, int max_y)
{
    HtGeom g;
    g.cs = P.cell_size;
    g.c = P.cos_a;
    g.s = P.sin_a;
    g.e = P.exponent;
    g.mn = P.min_dot;
    g.span = P.max_dot - P.min_dot;  // the reference's Python scalar (max_dot_size - min_dot_size)
    g.sharp = P.sharpness;
    g.sharpen = P.sharpness != 1.0;
    g.cls = P.exp_class;
    g.shape = P.shape;
    g.cx_min = cx_min;
    g.cy_min = cy_min;
    g.max_x = max_x;
    g.max_y = max_y;
    g.h = h;
    g.w = w;
    g.paper = P.paper_idx;
    g.fix_idx = P.exp_class == DP_HT_EXP_POW ? P.fix_idx_dev : nullptr;
    g.fix_thr = P.exp_class == DP_HT_EXP_POW ? P.fix_thr_dev : nullptr;
    g.n_fix = P.exp_class == DP_HT_EXP_POW ? P.n_fix : 0;
    return g;
}

int launch_halftone(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, const PalDev &pal,
                    const dp_halftone_params &P, void *ws, size_t ws_bytes, hipStream_t s)
{
    int cx_min, cy_min, max_x, max_y;
    size_t S;
    const int rc = halftone_grid(h, w, P, cx_min, cy_min, max_x, max_y, S);
    if (rc != DP_OK) return rc;
    const int64_t G = halftone_group(n_frames, S);
    if (ws_bytes < kHeadBytes + (size_t)G * S * 20) {
        set_error("dp_halftone_u8: workspace too small (see dp_halftone_workspace_bytes)");
        return DP_EWORKSPACE;
    }
    const HtGeom g = make_geom(h, w, P, cx_min, cy_min, max_x, max_y);
    uint32_t *n_ties = reinterpret_cast<uint32_t *>(ws);
    uint32_t *cells = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ws) + kHeadBytes);
    uint32_t *ties = cells + (size_t)G * S * 4;
    const size_t npx = (size_t)h * (size_t)w;
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    const bool big = pal.n_inner > kQueueSmall;
    ProfMark *pm = prof_begin(s);
    for (int64_t f0 = 0; f0 < n_frames; f0 += G) {
        const unsigned gn = (unsigned)(n_frames - f0 < G ? n_frames - f0 : G);
        const uint8_t *fin = in + (size_t)f0 * npx * 3;
        uint8_t *fout = out + (size_t)f0 * npx * 3;
        DP_HIP(hipMemsetAsync(ws, 0, kHeadBytes + (size_t)gn * S * 16, s));
        hipLaunchKernelGGL(ht_cell_kernel, dim3((unsigned)(tiles_x * tiles_y), gn), dim3(kBlock), 0, s, fin, cells, g,
                           pal.lut_in, tiles_x, S);
        hipLaunchKernelGGL(ht_colour_kernel, dim3((unsigned)((S + kBlock - 1) / kBlock), gn), dim3(kBlock), 0, s, cells, S,
                           pal, ties, n_ties);
        if (pal.K > kLeafSize) {
            if (big)
                hipLaunchKernelGGL(ht_tie_kernel<kQueueLarge>, dim3(64), dim3(64), 0, s, cells, ties, n_ties, pal);
            else
                hipLaunchKernelGGL(ht_tie_kernel<kQueueSmall>, dim3(64), dim3(64), 0, s, cells, ties, n_ties, pal);
        }
        hipLaunchKernelGGL(ht_ink_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock), gn), dim3(kBlock), 0, s, fin, fout,
                           cells, g, pal.lut_in, pal.out_rgb, S);
    }
    prof_end(pm, s);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int launch_halftone_pow_flags(int h, int w, const dp_halftone_params &P, int32_t *idx, int64_t cap,
                              unsigned long long *count, hipStream_t s)
{
    int cx_min, cy_min, max_x, max_y;
    size_t S;
    const int rc = halftone_grid(h, w, P, cx_min, cy_min, max_x, max_y, S);
    if (rc != DP_OK) return rc;
    DP_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    if (P.exp_class != DP_HT_EXP_POW) return DP_OK;
    const HtGeom g = make_geom(h, w, P, cx_min, cy_min, max_x, max_y);
    const size_t npx = (size_t)h * (size_t)w;
    hipLaunchKernelGGL(ht_flags_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, g, idx, cap,
                       count);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

}  // namespace dp
