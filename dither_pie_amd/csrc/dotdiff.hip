// Dot diffusion (include/ditherpie_hip_dotdiff.h): error diffusion in the order of a tiled class matrix; the error of a pixel
// goes to its neighbours of a higher class only, so a pixel depends on nothing farther away than reach(M) <= 16 king moves
// and the image is cut into tiles that are diffused independently and exactly.
//
// dotdiff_kernel<T, BLOCK>  one workgroup owns a T x T tile of one frame and works on the tile plus a halo of 16 pixels on
//   each side, clipped to the image (a region of at most (T + 32)^2 pixels whose origin is a multiple of 16, hence of m).
//   Every pixel of the region has one 12-byte slot in LDS.  The slot first holds the pixel's source colour (through lut_in);
//   once the pixel is quantised it holds what the pixel hands on: trunc(e * wt * strength / (256 W)) per channel for wt = 1
//   (a diagonal neighbour) and wt = 2 (an orthogonal one), six int16.  The workgroup walks the LEVELS of the matrix
//   (host_logic.h: dotdiff_levels; reach + 1 steps, 15 for the default matrix, instead of m * m classes) with a barrier
//   between two levels.  Pixels of one level are never neighbours: a lane takes one of them, PULLS the shares of its
//   neighbours of a lower class (they are of lower levels: finished, behind a barrier), quantises by one gather from the
//   palette's 2^24-entry nearest table (pattern.hip) and writes its own slot -- no atomics, and the order of the integer
//   additions does not matter.  The work of a level is dense: item i is cell i % n of the level's n cells in matrix tile
//   i / n of the region.  Pixels that miss a neighbour beyond the region are wrong, but a wrong value travels along a path of
//   increasing classes, which is too short to bring it from beyond the halo into the tile.  The tile's
//   pixels leave their luminance rank in LDS; at the end the tile is written row by row, consecutive lanes consecutive bytes.
//   A workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is capped, so that an image of 2^30 pixels in
//   one column (2^24 tiles) needs no grid of that size.
// Tile edge: T = 64 with 1024 lanes (114.8 KB of LDS: one workgroup per CU, 2.25 times the pixels).  T = 48 (512 lanes, two per
// CU, 2.8 times) and T = 32 (256 lanes, three per CU, 4 times) measured 2-5 % and about 50 % slower in every case and are
// not compiled (DESIGN.md 4.3e has the figures).
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_dotdiff.h"
#include "pattern_tab.hip.h"

namespace dp {
namespace {

static_assert(kDotDiffMaxReach == DP_DOTDIFF_MAX_REACH, "the halo of the kernel is the header's limit");
constexpr int kDotTile = 64;               // the tile edge (backend.DOTDIFF_TILE)
constexpr int kDotBlock = 1024;            // lanes of a workgroup
constexpr uint32_t kDotGridCap = 1u << 20; // workgroups per frame at most; the rest of the tiles by the loop in the kernel
constexpr size_t kLdsBytes = 160 * 1024;

// The class matrix and its level schedule, by value (kernel arguments; staged in LDS by the first lanes)
struct DotDev {
    uint8_t cls[kDotDiffMaxCells];
    uint8_t order[kDotDiffMaxCells];
    uint16_t start[kDotDiffMaxReach + 2];
    int m, log2m, n_levels;
};

__device__ __forceinline__ uint32_t nearest_rank(const PatDev &pd, const uint32_t r, const uint32_t g, const uint32_t b)
{
#ifdef DP_EXPERIMENTS
    if (!pd.brick) return pd.tab[tab_addr<false>(r, g, b)];
#endif
    return pd.tab[tab_addr<true>(r, g, b)];
}

__device__ __forceinline__ int lo16(const uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int hi16(const uint32_t v) { return (int)v >> 16; }

// trunc(e * wt * strength / (256 W)) for wt = 1, 2 as two int16 fields.  |e| <= 4080, strength <= 256: a = |e| wt strength >> 8
// <= 8160.  floor(a / W) = (a * mg) >> 18 with mg = ceil(2^18 / W): the excess a (mg - 2^18 / W) / 2^18 < 8160 / 2^18 < 1 / 12
// <= 1 / W, and a * mg <= 8160 * 2^18 < 2^32.  mg = 0 for W = 0: a baron drops its error.
__device__ __forceinline__ void shares(const int e, const uint32_t strength, const uint32_t mg, uint32_t &d1, uint32_t &d2)
{
    const uint32_t ae = (uint32_t)(e < 0 ? -e : e);
    const uint32_t q1 = (((ae * strength) >> 8) * mg) >> 18, q2 = (((2u * ae * strength) >> 8) * mg) >> 18;
    d1 = (uint32_t)(e < 0 ? -(int)q1 : (int)q1) & 0xffffu;
    d2 = (uint32_t)(e < 0 ? -(int)q2 : (int)q2) & 0xffffu;
}

// the arguments of a MASKED instance behind strength: the mask (n_frames x h x w bytes, non-zero = transparent) and fill (r | g << 8 | b << 16)
__device__ __forceinline__ const uint8_t *dot_mask_of(const uint8_t *mask_all, uint32_t) { return mask_all; }
__device__ __forceinline__ uint32_t dot_fill_of(const uint8_t *, const uint32_t fill) { return fill; }

// MASK is empty -- the instance of include/ditherpie_hip_dotdiff.h, whose argument list and code are what they were before the pack
// existed -- or (const uint8_t *, uint32_t): the MASKED instance of include/ditherpie_hip_alpha.h.  There bit 24 of a slot's word 0
// says "transparent" while the slot still holds the source colour: a neighbour of greater class is of a later level, so its flag is
// readable when W is formed (a neighbour beyond the region has no slot: its mask byte is read from memory, which only pixels on the
// region's edge do).  A transparent pixel hands on nothing (a slot of zeros) and its output bytes are `fill`.  No LDS is added.
// Why a pack and not a `bool MASKED` with two trailing arguments: a trailing kernel argument, used or not, moves the hidden arguments
// (the group size the runtime passes behind the explicit ones), which changes an immediate in the unmasked instances; with an empty
// pack their argument list is byte for byte the old one and their gfx950 instruction streams are unchanged (DESIGN.md 4.4 has the
// comparison).  Whoever adds a trailing argument to this kernel moves them for every instance and repeats that comparison.
template <int T, int BLOCK, typename... MASK>
__global__ __launch_bounds__(BLOCK) void dotdiff_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int h, const int w,
                                                        const uint32_t ntx, const uint32_t ntiles, const PatDev pd,
                                                        const uint8_t *__restrict__ lut, const DotDev dd, const uint32_t strength, const MASK... mask_args)
{
    constexpr bool MASKED = sizeof...(MASK) != 0;
    static_assert(sizeof...(MASK) == 0 || sizeof...(MASK) == 2, "no mask arguments, or the mask and the fill");
    constexpr int R = kDotDiffMaxReach, RS = T + 2 * R, NPX = RS * RS, WAVES = BLOCK / 64;
    static_assert(T % 16 == 0 && RS % 16 == 0, "the region's origin is a multiple of every matrix size");
    __shared__ uint32_t s_px[NPX * 3];   // the slots: source colour r | g<<8 | b<<16 in word 0, then d1.r | d1.g<<16, d1.b | d2.r<<16, d2.g | d2.b<<16
    __shared__ uint32_t s_c[256];        // by rank: trunc(pal_f32), r | g<<8 | b<<16
    __shared__ uint32_t s_out[256];      // by rank: the output bytes
    __shared__ uint8_t s_rank[T * T];    // the tile's result
    __shared__ uint8_t s_lut[256], s_cls[kDotDiffMaxCells], s_order[kDotDiffMaxCells];
    constexpr size_t kLds = sizeof(uint32_t) * (NPX * 3 + 512) + T * T + 256 + 2 * kDotDiffMaxCells;
    static_assert(kLds <= kLdsBytes, "one workgroup per CU fits its LDS");

    for (int i = threadIdx.x; i < 256; i += BLOCK) {
        s_c[i] = i < pd.K ? pd.c_rank[i] : 0u;
        s_out[i] = i < pd.K ? pd.out_rank[i] : 0u;
        s_lut[i] = lut ? lut[i] : (uint8_t)i;
        s_cls[i] = dd.cls[i];
        s_order[i] = dd.order[i];
    }
    const int log2m = dd.log2m, mm = dd.m - 1;
    const uint32_t ntr = (uint32_t)RS >> log2m;   // matrix tiles along one side of the region
    // ti / ntr = (ti * ceil(2^20 / ntr)) >> 20 for ti < ntr^2: the excess ti / 2^20 stays below 1 / ntr as ntr^3 < 2^20 (ntr <= RS / 2)
    static_assert((RS / 2) * (RS / 2) * (RS / 2) < (1 << 20), "the division by the tiles per side");
    const uint32_t ntr_inv = ((1u << 20) + ntr - 1u) / ntr;
    const size_t fbase = (size_t)blockIdx.y * 3u * (size_t)h * (size_t)w;
    const uint8_t *fin = in + fbase;
    uint8_t *fout = out + fbase;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(s_px);
    const uint8_t *__restrict__ fmask = nullptr;
    uint32_t fill = 0u;
    if constexpr (MASKED) {
        fmask = dot_mask_of(mask_args...) + (size_t)blockIdx.y * (size_t)h * (size_t)w;
        fill = dot_fill_of(mask_args...);
    }

    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ty0 = (int)(tile / ntx) * T, tx0 = (int)(tile % ntx) * T;        // the tile's first pixel; inside the image
        const int ry0 = max(ty0 - R, 0), rx0 = max(tx0 - R, 0);                    // the region's
        const int rh = min(RS, h - ry0), rw = min(RS, w - rx0);                    // ... and its size inside the image
        __syncthreads();   // the tables are staged; the previous tile is written

        // the region's source bytes through lut_in: a wave per row, consecutive lanes consecutive bytes.  All loads of a lane
        // are issued before the first is used (ROWS * CHUNKS registers): one trip to memory per tile, not one per byte
        {
            constexpr int ROWS = (RS + WAVES - 1) / WAVES, CHUNKS = (3 * RS + 63) / 64;
            uint8_t v[ROWS][CHUNKS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = wave + r * WAVES;
                const uint8_t *src = fin + ((size_t)(ry0 + min(row, rh - 1)) * (size_t)w + (size_t)rx0) * 3u;
#pragma unroll
                for (int j = 0; j < CHUNKS; ++j) {
                    const int b = lane + 64 * j;
                    v[r][j] = row < rh && b < 3 * rw ? src[b] : (uint8_t)0;
                }
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = wave + r * WAVES;
#pragma unroll
                for (int j = 0; j < CHUNKS; ++j) {
                    const int b = lane + 64 * j, px = b / 3, ch = b - 3 * px;
                    if (row < rh && b < 3 * rw) s_bytes[(row * RS + px) * 12 + ch] = s_lut[v[r][j]];
                }
            }
            if constexpr (MASKED) {   // the flags: byte 3 of every slot of the region
                constexpr int MCHUNKS = (RS + 63) / 64;
                uint8_t mv[ROWS][MCHUNKS];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int row = wave + r * WAVES;
                    const uint8_t *src = fmask + (size_t)(ry0 + min(row, rh - 1)) * (size_t)w + (size_t)rx0;
#pragma unroll
                    for (int j = 0; j < MCHUNKS; ++j) {
                        const int px = lane + 64 * j;
                        mv[r][j] = row < rh && px < rw ? src[px] : (uint8_t)0;
                    }
                }
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int row = wave + r * WAVES;
#pragma unroll
                    for (int j = 0; j < MCHUNKS; ++j) {
                        const int px = lane + 64 * j;
                        if (row < rh && px < rw) s_bytes[(row * RS + px) * 12 + 3] = mv[r][j] ? (uint8_t)1 : (uint8_t)0;
                    }
                }
            }
        }
        __syncthreads();

        for (int level = 0; level < dd.n_levels; ++level) {
            const uint32_t l0 = dd.start[level], nl = dd.start[level + 1] - l0, items = nl * ntr * ntr;
            // i / nl = umulhi(i, ceil(2^32 / nl)) for i < 2^24 (the excess i / 2^32 stays below 1 / nl); nl = 1 has no such word
            const uint32_t nl_inv = (uint32_t)((0x100000000ull + nl - 1u) / nl);
            for (uint32_t i = threadIdx.x; i < items; i += BLOCK) {
                const uint32_t ti = nl == 1u ? i : __umulhi(i, nl_inv), ci = i - ti * nl;
                const uint32_t tyr = (ti * ntr_inv) >> 20, txr = ti - tyr * ntr;
                const uint32_t cell = s_order[l0 + ci], cls = s_cls[cell];
                const int ly = (int)(tyr << log2m) + (int)(cell >> log2m), lx = (int)(txr << log2m) + (int)(cell & (uint32_t)mm);
                if (ly >= rh || lx >= rw) continue;                               // beyond the image
                const int gy = ry0 + ly, gx = rx0 + lx;
                if constexpr (MASKED) {
                    uint32_t *own = &s_px[(ly * RS + lx) * 3];
                    if (own[0] >> 24) {   // transparent: it hands on nothing; its bytes come from `fill` at the end
                        own[0] = own[1] = own[2] = 0u;
                        continue;
                    }
                }
                int ar = 0, ag = 0, ab = 0;
                uint32_t W = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int dy = k < 3 ? -1 : (k < 5 ? 0 : 1), dx = k < 3 ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
                    const bool orth = dy == 0 || dx == 0;
                    const int ngy = gy + dy, ngx = gx + dx, ny = ly + dy, nx = lx + dx;
                    if (ngy < 0 || ngy >= h || ngx < 0 || ngx >= w) continue;     // not in the image
                    const uint32_t ncls = s_cls[((ngy & mm) << log2m) | (ngx & mm)];
                    if (ncls > cls) {
                        if constexpr (MASKED) {   // E holds the opaque neighbours only
                            const bool inside = ny >= 0 && nx >= 0 && ny < rh && nx < rw;
                            const bool hidden = inside ? (s_px[(ny * RS + nx) * 3] >> 24) != 0u : fmask[(size_t)ngy * (size_t)w + (size_t)ngx] != 0;
                            W += hidden ? 0u : (orth ? 2u : 1u);
                        } else {
                            W += orth ? 2u : 1u;
                        }
                    } else if (ny >= 0 && nx >= 0) {                              // (ny < rh and nx < rw: it is in the image)
                        const uint32_t *q = &s_px[(ny * RS + nx) * 3];
                        if (orth) {
                            const uint32_t w1 = q[1], w2 = q[2];
                            ar += hi16(w1);
                            ag += lo16(w2);
                            ab += hi16(w2);
                        } else {
                            const uint32_t w0 = q[0], w1 = q[1];
                            ar += lo16(w0);
                            ag += hi16(w0);
                            ab += lo16(w1);
                        }
                    }
                }
                uint32_t *slot = &s_px[(ly * RS + lx) * 3];
                const uint32_t c = slot[0];   // (MASKED: bit 24 is clear, the pixel is opaque)
                const int ur = min(max(16 * (int)(c & 255u) + ar, 0), 4080), ug = min(max(16 * (int)((c >> 8) & 255u) + ag, 0), 4080),
                          ub = min(max(16 * (int)((c >> 16) & 255u) + ab, 0), 4080);
                const uint32_t rk = nearest_rank(pd, (uint32_t)(ur + 8) >> 4, (uint32_t)(ug + 8) >> 4, (uint32_t)(ub + 8) >> 4);   // < 2^24 by the clamp
                const uint32_t cc = s_c[rk];
                const uint32_t mg = W ? (262144u + W - 1u) / W : 0u;
                uint32_t r1, r2, g1, g2, b1, b2;
                shares(ur - 16 * (int)(cc & 255u), strength, mg, r1, r2);
                shares(ug - 16 * (int)((cc >> 8) & 255u), strength, mg, g1, g2);
                shares(ub - 16 * (int)(cc >> 16), strength, mg, b1, b2);
                slot[0] = r1 | (g1 << 16);
                slot[1] = b1 | (r2 << 16);
                slot[2] = g2 | (b2 << 16);
                const int oy = gy - ty0, ox = gx - tx0;
                if (oy >= 0 && oy < T && ox >= 0 && ox < T) s_rank[oy * T + ox] = (uint8_t)rk;
            }
            __syncthreads();
        }

        // the tile, clipped to the image: a wave per row, consecutive lanes consecutive bytes
        const int th = min(T, h - ty0), tw = min(T, w - tx0);
        for (int row = wave; row < th; row += WAVES) {
            uint8_t *dst = fout + ((size_t)(ty0 + row) * (size_t)w + (size_t)tx0) * 3u;
            for (int b = lane; b < 3 * tw; b += 64) {
                const int px = b / 3, ch = b - 3 * px;
                if constexpr (MASKED) {
                    const bool hidden = fmask[(size_t)(ty0 + row) * (size_t)w + (size_t)(tx0 + px)] != 0;
                    dst[b] = (uint8_t)((hidden ? fill : s_out[s_rank[row * T + px]]) >> (8 * ch));
                } else {
                    dst[b] = (uint8_t)(s_out[s_rank[row * T + px]] >> (8 * ch));
                }
            }
        }
    }
}

// mask: nullptr for the unmasked instance, else n_frames x h x w bytes and the MASKED one (masked pixels become `fill`)
int launch_dotdiff(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, const PatDev &pd, const uint8_t *lut,
                   const DotDev &dd, int strength, hipStream_t s, const uint8_t *mask = nullptr, const uint32_t fill = 0)
{
    constexpr int T = kDotTile;
    const size_t frame = 3 * (size_t)h * (size_t)w;
    const uint32_t ntx = ((uint32_t)w + T - 1) / T, nty = ((uint32_t)h + T - 1) / T, ntiles = ntx * nty;   // h * w <= 2^30: no overflow
    uint32_t cap = kDotGridCap;   // (the experiments build can lower it, so that a small image walks the tile loop)
    if (const char *e = exp_env("DP_DOTDIFF_GRID_CAP")) cap = (uint32_t)std::min(std::max(std::atoi(e), 1), (int)kDotGridCap);
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const uint32_t nf = (uint32_t)std::min<int64_t>(65535, n_frames - f0);
        ProfMark *pm = prof_begin(s);
        if (mask)
            hipLaunchKernelGGL((dotdiff_kernel<T, kDotBlock, const uint8_t *, uint32_t>), dim3(std::min(ntiles, cap), nf), dim3(kDotBlock), 0, s,
                               in + (size_t)f0 * frame, out + (size_t)f0 * frame, h, w, ntx, ntiles, pd, lut, dd, (uint32_t)strength,
                               mask + (size_t)f0 * (frame / 3), fill);
        else
            hipLaunchKernelGGL((dotdiff_kernel<T, kDotBlock>), dim3(std::min(ntiles, cap), nf), dim3(kDotBlock), 0, s, in + (size_t)f0 * frame,
                               out + (size_t)f0 * frame, h, w, ntx, ntiles, pd, lut, dd, (uint32_t)strength);
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

}  // namespace

int dotdiff_call(const char *fn, const bool masked, const uint8_t *in_dev, const uint8_t *mask_dev, const uint32_t fill, uint8_t *out_dev, int64_t n_frames,
                 int h, int w, const dp_palette *pal, const uint8_t *classes_host, int m, int strength256, void *stream)
{
    const bool sizes_ok = n_frames >= 0 && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)1 << 30;
    if (!pal || !classes_host || !sizes_ok || (n_frames > 0 && (!in_dev || !out_dev || (masked && !mask_dev)))) {
        set_error("%s: bad argument (pointers, n_frames >= 0, h, w >= 1, h * w <= 2^30)", fn);
        return DP_EINVAL;
    }
    if (m != 2 && m != 4 && m != 8 && m != 16) {
        set_error("%s: the class matrix must be 2, 4, 8 or 16 wide, not %d", fn, m);
        return DP_EINVAL;
    }
    if (!dotdiff_matrix_ok(classes_host, m)) {
        set_error("%s: the class matrix is not a permutation of 0 .. %d", fn, m * m - 1);
        return DP_EINVAL;
    }
    if (strength256 < 0 || strength256 > 256) {
        set_error("%s: strength256 must lie in 0 .. 256, not %d", fn, strength256);
        return DP_EINVAL;
    }
    if (in_dev && out_dev == in_dev) {
        set_error("%s: out_dev must not be in_dev (tiles read a halo of their neighbours' input)", fn);
        return DP_EINVAL;
    }
    if (masked && n_frames > 0) {
        const size_t px = (size_t)n_frames * (size_t)h * (size_t)w;
        const uintptr_t o = (uintptr_t)out_dev, i = (uintptr_t)in_dev, k = (uintptr_t)mask_dev;
        if ((o < i + 3u * px && i < o + 3u * px) || (o < k + px && k < o + 3u * px)) {
            set_error("%s: out_dev must not overlap in_dev or mask_dev", fn);
            return DP_EINVAL;
        }
    }
    int rc = pattern_check_palette(fn, pal);
    if (rc != DP_OK) return rc;
    int level[kDotDiffMaxCells];
    const int reach = dotdiff_levels(classes_host, m, level);
    if (reach > kDotDiffMaxReach) {
        set_error("%s: the class matrix has reach %d, at most %d is supported", fn, reach, kDotDiffMaxReach);
        return DP_EUNSUPPORTED;
    }
    if (n_frames == 0) return DP_OK;
    DotDev dd;
    DotDiffSchedule sch;
    dotdiff_schedule(level, m, reach, sch);
    for (int i = 0; i < kDotDiffMaxCells; ++i) {
        dd.cls[i] = i < m * m ? classes_host[i] : (uint8_t)0;
        dd.order[i] = sch.order[i];
    }
    for (int i = 0; i < kDotDiffMaxReach + 2; ++i) dd.start[i] = sch.start[i];
    dd.m = m;
    dd.log2m = m == 2 ? 1 : (m == 4 ? 2 : (m == 8 ? 3 : 4));
    dd.n_levels = sch.n_levels;
    rc = pattern_ensure_table(pal, (hipStream_t)stream);
    if (rc != DP_OK) return rc;
    const uint8_t *lut;
    {
        dp_palette *p = const_cast<dp_palette *>(pal);
        std::lock_guard<std::mutex> lock(p->dev_mu);
        lut = p->dev.lut_in;
    }
    return launch_dotdiff(in_dev, out_dev, n_frames, h, w, pattern_snapshot(pal), lut, dd, strength256, (hipStream_t)stream, masked ? mask_dev : nullptr, fill);
}

}  // namespace dp

using namespace dp;

extern "C" {

int dp_dotdiff_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, const dp_palette *pal,
                  const uint8_t *classes_host, int m, int strength256, void *stream)
{
    return dotdiff_call("dp_dotdiff_u8", false, in_dev, nullptr, 0u, out_dev, n_frames, h, w, pal, classes_host, m, strength256, stream);
}

}  // extern "C"
