// Pattern (Knoll) dithering (include/ditherpie_hip_pattern.h): per pixel n = m * m nearest-colour searches build a candidate
// list whose mean approximates the pixel, the Bayer rank matrix picks the B[y][x]-th of the list in luminance order.
//
// The searches are gathers from an exact table of nearest(q) over all 2^24 colours, one byte per colour, holding the
// luminance RANK of the entry (position in the order by (L, index)): candidates are then sortable bytes and the palette
// colours are kept by rank.  The table is built by the library's own nearest-only path (launch_ordered, DP_MODE_NEAREST,
// brute-force pass + KD-tree fix-up of the ties) over the identity colours, with a copy of the palette record whose output
// "colours" are the ranks, whose lut_in is dropped and whose accelerator tables are left out (those kernels write the
// palette colours themselves, not out_rgb): the table is that path, scipy's tie order included.  For a palette with a colour
// metric (metric.hip) the table is packed from the metric's own top-2 table instead: only nearest(q) changes.
//
// pattern_identity_kernel  the colours of 2^22 consecutive table addresses as packed RGB pixels (four per lane)
// pattern_pack_kernel      byte 0 of each pixel of the nearest-only output -> the table (four per lane, one dword store)
// pattern_kernel<M, BRICK> one lane owns PPL pixels (2 at m = 8, 4 below; 256 apart, so the byte loads and stores of a
//                          wave touch consecutive pixels).  n iterations, fully unrolled, the pixels of a lane interleaved
//                          so that their dependent gathers overlap; -C[] and out_colors by rank and lut_in in LDS (5 KB);
//                          the candidates packed four per register (no runtime-indexed array: nothing in scratch).  The
//                          selection needs no sort: a binary search over the rank value, one step per bit of K - 1,
//                          each counting the candidates below the probe with two 16-bit-field adds per register.
// Table layout: 4 x 4 x 4 colours per 64-byte line (BRICK).  Measured against the plain r | g<<8 | b<<16 order in one session
// (tools/bench_scripts/pattern_bench.py; DESIGN.md 4.3d has the figures): the bricks cost ten address instructions per search
// instead of two but are 18 % / 3 % faster at m = 8 with 256 colours (1080p / 4K) and 13 % slower at m = 4 with 16 colours, the
// cheapest case; they are the product's layout.  The plain order is compiled into the experiments build only
// (DP_PATTERN_PLAIN=1), so that the A/B can be repeated.
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_pattern.h"
#include "pattern_tab.hip.h"

namespace dp {
namespace {

constexpr int kPatBlock = 256;
constexpr size_t kTabBytes = (size_t)DP_PATTERN_TABLE_BYTES;
constexpr int kBuildSide = 2048;                                   // the table is built in "frames" of 2048 x 2048 colours
constexpr uint32_t kBuildPx = (uint32_t)kBuildSide * kBuildSide;   // 2^22: four of them
constexpr size_t kSideBytes = 3 * 256 * sizeof(uint32_t);          // c_rank, out_rank, the ranks by index (build only)

// px: kBuildPx packed RGB pixels, 4-byte aligned; pixel i = the colour of table address a0 + i
template <bool BRICK>
__global__ __launch_bounds__(kPatBlock) void pattern_identity_kernel(uint32_t *__restrict__ px, const uint32_t a0)
{
    const uint32_t t = blockIdx.x * kPatBlock + threadIdx.x;   // the grid covers kBuildPx / 4 lanes exactly
    const uint32_t a = a0 + 4u * t;
    const uint32_t c0 = tab_colour<BRICK>(a), c1 = tab_colour<BRICK>(a + 1u), c2 = tab_colour<BRICK>(a + 2u), c3 = tab_colour<BRICK>(a + 3u);
    px[3u * t] = c0 | (c1 << 24);
    px[3u * t + 1u] = (c1 >> 8) | (c2 << 16);
    px[3u * t + 2u] = (c2 >> 16) | (c3 << 8);
}

// tab4[t] = byte 0 of pixels 4t .. 4t+3 of the nearest-only output (the rank: the "red" byte of the substituted out_rgb)
__global__ __launch_bounds__(kPatBlock) void pattern_pack_kernel(const uint32_t *__restrict__ px, uint32_t *__restrict__ tab4)
{
    const uint32_t t = blockIdx.x * kPatBlock + threadIdx.x;
    const uint32_t w0 = px[3u * t], w1 = px[3u * t + 1u], w2 = px[3u * t + 2u];
    tab4[t] = (w0 & 255u) | ((w0 >> 24) << 8) | (((w1 >> 16) & 255u) << 16) | (((w2 >> 8) & 255u) << 24);
}

// B_m[y mod m][x mod m]: B_2 = [[0, 2], [3, 1]] is ((x ^ y) << 1 | y) of the one bit; B_2m = 4 B_m(low bits) + B_2(top bit)
template <int M>
__device__ __forceinline__ uint32_t bayer_rank(const uint32_t y, const uint32_t x)
{
    constexpr int BITS = M == 8 ? 3 : (M == 4 ? 2 : 1);
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < BITS; ++j) {
        const uint32_t yb = (y >> j) & 1u, xb = (x >> j) & 1u;
        r |= (((xb ^ yb) << 1) | yb) << (2 * (BITS - 1 - j));
    }
    return r;
}

// in and out may be the same buffer (no __restrict__): a lane reads its pixels before it writes them
template <int M, bool BRICK>
__global__ __launch_bounds__(kPatBlock) void pattern_kernel(const uint8_t *in, uint8_t *out, const uint32_t hw, const uint32_t w,
                                                            const uint32_t ym, const uint32_t xm, const PatDev pd,
                                                            const uint8_t *__restrict__ lut, const int strength)
{
    constexpr int N = M * M, NW = N / 4, PPL = M == 8 ? 2 : 4;
    __shared__ int4 s_neg[256];      // by rank: {-C.r, -C.g, -C.b, 0}: one read of the 16-byte record per search (hipcc fetches
                                     // the 12 bytes in use, ds_read_b96), the update is three v_add3
    __shared__ uint32_t s_out[256];
    __shared__ uint8_t s_lut[256];
    for (int i = threadIdx.x; i < 256; i += kPatBlock) {
        const uint32_t cc = i < pd.K ? pd.c_rank[i] : 0u;
        s_neg[i] = make_int4(-(int)(cc & 255u), -(int)((cc >> 8) & 255u), -(int)(cc >> 16), 0);
        s_out[i] = i < pd.K ? pd.out_rank[i] : 0u;
        s_lut[i] = lut ? lut[i] : (uint8_t)i;
    }
    __syncthreads();

    const size_t fbase = (size_t)blockIdx.y * 3u * (size_t)hw;
    const uint8_t *fin = in + fbase;
    uint8_t *fout = out + fbase;
    const uint32_t p0 = blockIdx.x * (uint32_t)(kPatBlock * PPL) + threadIdx.x;

    int cr[PPL], cg[PPL], cb[PPL], er[PPL], eg[PPL], eb[PPL];
    uint32_t cand[PPL][NW];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const uint32_t p = p0 + (uint32_t)q * kPatBlock;
        uint32_t r = 0, g = 0, b = 0;
        if (p < hw) {
            const uint8_t *s = fin + (size_t)p * 3u;
            r = s[0];
            g = s[1];
            b = s[2];
        }
        cr[q] = (int)s_lut[r];
        cg[q] = (int)s_lut[g];
        cb[q] = (int)s_lut[b];
        er[q] = eg[q] = eb[q] = 0;
    }

#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            // c + floor(e * strength / 256) = (256 c + e * strength) >> 8: floor, not truncation, by the arithmetic shift
            // (|e| <= 64 * 255 and strength <= 256: a 24-bit multiply-add)
            const uint32_t tr = (uint32_t)min(max((__mul24(er[q], strength) + (cr[q] << 8)) >> 8, 0), 255);
            const uint32_t tg = (uint32_t)min(max((__mul24(eg[q], strength) + (cg[q] << 8)) >> 8, 0), 255);
            const uint32_t tb = (uint32_t)min(max((__mul24(eb[q], strength) + (cb[q] << 8)) >> 8, 0), 255);
            const uint32_t rk = pd.tab[tab_addr<BRICK>(tr, tg, tb)];   // < 2^24 by the clamp
            const int4 nc = s_neg[rk];
            er[q] += cr[q] + nc.x;
            eg[q] += cg[q] + nc.y;
            eb[q] += cb[q] + nc.z;
            if ((i & 3) == 0) cand[q][i >> 2] = rk;
            else cand[q][i >> 2] |= rk << (8 * (i & 3));
        }
    }

    // ranks are below K: the search needs only the bits of K - 1 (wave-uniform)
    const int nbits = pd.K > 1 ? 32 - __clz(pd.K - 1) : 0;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const uint32_t p = p0 + (uint32_t)q * kPatBlock;
        if (p >= hw) continue;
        const uint32_t y = p / w, x = p - y * w;
        const uint32_t want = bayer_rank<M>(y + ym, x + xm);
        // the want-th smallest candidate (0-based) = the largest v with #(candidates < v) <= want, bit by bit.
        // Per register: the bytes as two pairs of 16-bit fields holding 255 - byte; v + (255 - byte) has bit 8 set iff
        // byte < v, and the flags (bits 8 and 24) add up in place: at most 64 << 24 < 2^32.
        uint32_t nlo[NW], nhi[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const uint32_t nw = ~cand[q][j];
            nlo[j] = nw & 0x00ff00ffu;
            nhi[j] = (nw >> 8) & 0x00ff00ffu;
        }
        uint32_t ans = 0;
#pragma unroll
        for (int bit = 7; bit >= 0; --bit) {
            if (bit >= nbits) continue;
            const uint32_t v = ans | (1u << bit), v2 = v * 0x00010001u;
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < NW; ++j) acc += ((nlo[j] + v2) & 0x01000100u) + ((nhi[j] + v2) & 0x01000100u);
            const uint32_t below = ((acc >> 8) & 0xffu) + (acc >> 24);
            if (below <= want) ans = v;
        }
        const uint32_t c = s_out[ans];
        uint8_t *o = fout + (size_t)p * 3u;
        o[0] = (uint8_t)c;
        o[1] = (uint8_t)(c >> 8);
        o[2] = (uint8_t)(c >> 16);
    }
}

template <int M>
void launch_pattern_m(const uint8_t *in, uint8_t *out, uint32_t frames, uint32_t hw, uint32_t w, uint32_t ym, uint32_t xm,
                      const PatDev &pd, const uint8_t *lut, int strength, hipStream_t s)
{
    constexpr int PPL = M == 8 ? 2 : 4;
    const dim3 grid((hw + kPatBlock * PPL - 1) / (kPatBlock * PPL), frames);
#ifdef DP_EXPERIMENTS
    if (!pd.brick) {
        hipLaunchKernelGGL((pattern_kernel<M, false>), grid, dim3(kPatBlock), 0, s, in, out, hw, w, ym, xm, pd, lut, strength);
        return;
    }
#endif
    hipLaunchKernelGGL((pattern_kernel<M, true>), grid, dim3(kPatBlock), 0, s, in, out, hw, w, ym, xm, pd, lut, strength);
}

int launch_pattern(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, int y0, int x0, const PatDev &pd,
                   const uint8_t *lut, int matrix, int strength, hipStream_t s)
{
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const uint32_t nf = (uint32_t)std::min<int64_t>(65535, n_frames - f0);
        const uint8_t *in_c = in + (size_t)f0 * hw * 3;
        uint8_t *out_c = out + (size_t)f0 * hw * 3;
        const uint32_t ym = (uint32_t)(y0 % matrix), xm = (uint32_t)(x0 % matrix);
        ProfMark *pm = prof_begin(s);
        if (matrix == 2) launch_pattern_m<2>(in_c, out_c, nf, hw, (uint32_t)w, ym, xm, pd, lut, strength, s);
        else if (matrix == 4) launch_pattern_m<4>(in_c, out_c, nf, hw, (uint32_t)w, ym, xm, pd, lut, strength, s);
        else launch_pattern_m<8>(in_c, out_c, nf, hw, (uint32_t)w, ym, xm, pd, lut, strength, s);
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

// The four nearest-only passes over the identity colours; `d` is the stripped palette record (see the head of the file).
int fill_table(const PalDev &d, uint8_t *tab, int brick, hipStream_t s)
{
    const size_t frame = 3 * (size_t)kBuildPx, ws_bytes = dp_ordered_workspace_bytes(1, kBuildSide, kBuildSide);
    uint8_t *scratch = nullptr;   // identity colours | nearest-only output | the ordered kernels' workspace; stream-ordered
    DP_HIP(hipMallocAsync((void **)&scratch, 2 * frame + ws_bytes, s));
    uint8_t *px_in = scratch, *px_out = scratch + frame, *ws = scratch + 2 * frame;
    int rc = DP_OK;
    for (uint32_t part = 0; part < (uint32_t)(kTabBytes / kBuildPx) && rc == DP_OK; ++part) {
        const uint32_t a0 = part * kBuildPx;
        const dim3 grid(kBuildPx / 4 / kPatBlock);
#ifdef DP_EXPERIMENTS
        if (!brick) hipLaunchKernelGGL(pattern_identity_kernel<false>, grid, dim3(kPatBlock), 0, s, reinterpret_cast<uint32_t *>(px_in), a0);
        else
#endif
            hipLaunchKernelGGL(pattern_identity_kernel<true>, grid, dim3(kPatBlock), 0, s, reinterpret_cast<uint32_t *>(px_in), a0);
        rc = launch_ordered(px_in, px_out, 1, kBuildSide, kBuildSide, 0, 0, d, DP_MODE_NEAREST, nullptr, 0.0f, 0, ws, ws_bytes, s);
        if (rc != DP_OK) break;
        hipLaunchKernelGGL(pattern_pack_kernel, grid, dim3(kPatBlock), 0, s, reinterpret_cast<const uint32_t *>(px_out),
                           reinterpret_cast<uint32_t *>(tab + a0));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "pattern table launch");
    }
    (void)hipFreeAsync(scratch, s);
    return rc;
}

}  // namespace

// K <= 256 and every palette value in [0, 255] (what trunc() and the clamp of the definitions assume); `fn` is the entry
// point that is refusing (dp_pattern_*, dp_dotdiff_u8)
int pattern_check_palette(const char *fn, const dp_palette *p)
{
    if (p->dev.K > 256) {
        set_error("%s: the nearest table supports at most 256 colours, the palette has %d", fn, p->dev.K);
        return DP_EUNSUPPORTED;
    }
    for (const double v : p->pts_host)
        if (!(v >= 0.0 && v <= 255.0)) {
            set_error("%s: the nearest table needs palette values in [0, 255], found %g", fn, v);
            return DP_EUNSUPPORTED;
        }
    return DP_OK;
}

PatDev pattern_snapshot(const dp_palette *pal_c)
{
    dp_palette *p = const_cast<dp_palette *>(pal_c);
    std::lock_guard<std::mutex> lock(p->dev_mu);
    return p->pat;
}

// Build the table once (under build_mu; the launches go to `s`, which is waited for before the table is published: another
// thread may use it on another stream at once).  A failed build leaves the palette without a table; the next call retries.
int pattern_ensure_table(const dp_palette *pal_c, hipStream_t s)
{
    dp_palette *p = const_cast<dp_palette *>(pal_c);
    std::lock_guard<std::mutex> lock(p->build_mu);
    if (p->pat.tab) return DP_OK;
    PalDev d;
    {
        std::lock_guard<std::mutex> dl(p->dev_mu);
        d = p->dev;
    }
    const int K = d.K;
    // host side: C[k] = trunc(pal), the order by (L, k), and the palette's output colours
    std::vector<uint32_t> c(K), l(K), order(K), orgb(K), side(3 * 256, 0u);
    for (int k = 0; k < K; ++k) {
        const uint32_t r = (uint32_t)p->pts_host[3 * k], g = (uint32_t)p->pts_host[3 * k + 1], b = (uint32_t)p->pts_host[3 * k + 2];
        c[k] = r | (g << 8) | (b << 16);
        l[k] = 299u * r + 587u * g + 114u * b;
        order[k] = (uint32_t)k;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return l[a] != l[b] ? l[a] < l[b] : a < b; });
    DP_HIP(hipMemcpy(orgb.data(), d.out_rgb, sizeof(uint32_t) * K, hipMemcpyDeviceToHost));
    for (int i = 0; i < K; ++i) {
        side[i] = c[order[i]];
        side[256 + i] = orgb[order[i]];
        side[512 + order[i]] = (uint32_t)i;   // rank of entry order[i]: what the nearest-only pass writes for it
    }
    void *blob = nullptr;
    DP_HIP(hipMalloc(&blob, kTabBytes + kSideBytes));
    uint8_t *tab = reinterpret_cast<uint8_t *>(blob);
    const uint32_t *side_dev = reinterpret_cast<const uint32_t *>(tab + kTabBytes);
    hipError_t e = hipMemcpy(tab + kTabBytes, side.data(), kSideBytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? DP_OK : hip_fail(e, "pattern table upload");
    const int brick = (exp_env("DP_PATTERN_PLAIN") && p->metric == 0) ? 0 : 1;
    if (rc == DP_OK) {
        if (K == 1) {   // every colour maps to the one entry, rank 0
            e = hipMemsetAsync(tab, 0, kTabBytes, s);
            if (e != hipSuccess) rc = hip_fail(e, "pattern table memset");
        } else if (p->metric != 0) {   // a metric palette (metric.hip): nearest(q) is its top-2 table's, one pack kernel; bricks always
            rc = metric_ensure_table_locked(p, s);
            if (rc == DP_OK) rc = launch_metric_rank_table(p->met, side_dev + 512, tab, s);
        } else {
            d.lut_in = nullptr;
            d.out_rgb = side_dev + 512;
            d.cell_tab = d.cell_tab4 = d.warp_tab = d.comp_tab = d.ftab = nullptr;   // the brute-force pass + tree fix-up
            d.cell_perm = d.cell_perm4 = nullptr;
            rc = fill_table(d, tab, brick, s);
        }
    }
    if (rc == DP_OK) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "pattern table build");
    }
    if (rc != DP_OK) {
        (void)hipFree(blob);
        return rc;
    }
    p->pat_blob = blob;
    std::lock_guard<std::mutex> dl(p->dev_mu);
    p->pat = PatDev{tab, side_dev, side_dev + 256, K, brick};
    return DP_OK;
}

}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_pattern_table_bytes(const dp_palette *pal)
{
    if (!pal || pal->dev.K > 256) return 0;
    for (const double v : pal->pts_host)
        if (!(v >= 0.0 && v <= 255.0)) return 0;
    return kTabBytes + kSideBytes;
}

int dp_pattern_prepare(dp_palette *pal)
{
    if (!pal) {
        set_error("dp_pattern_prepare: NULL palette");
        return DP_EINVAL;
    }
    const int rc = pattern_check_palette("dp_pattern_prepare", pal);
    if (rc != DP_OK) return rc;
    return pattern_ensure_table(pal, nullptr);
}

int dp_pattern_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, int y0, int x0, const dp_palette *pal,
                  int matrix, int strength256, void *stream)
{
    const bool sizes_ok = n_frames >= 0 && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)h * w <= (int64_t)1 << 30 &&
                          (int64_t)y0 + h <= (int64_t)1 << 30 && (int64_t)x0 + w <= (int64_t)1 << 30;
    if (!pal || !sizes_ok || (n_frames > 0 && (!in_dev || !out_dev))) {
        set_error("dp_pattern_u8: bad argument (pointers, n_frames >= 0, h, w >= 1, h * w <= 2^30, y0, x0 >= 0)");
        return DP_EINVAL;
    }
    if (matrix != 2 && matrix != 4 && matrix != 8) {
        set_error("dp_pattern_u8: matrix must be 2, 4 or 8, not %d", matrix);
        return DP_EINVAL;
    }
    if (strength256 < 0 || strength256 > 256) {
        set_error("dp_pattern_u8: strength256 must lie in 0 .. 256, not %d", strength256);
        return DP_EINVAL;
    }
    int rc = pattern_check_palette("dp_pattern_u8", pal);
    if (rc != DP_OK) return rc;
    if (n_frames == 0) return DP_OK;
    rc = pattern_ensure_table(pal, (hipStream_t)stream);
    if (rc != DP_OK) return rc;
    const uint8_t *lut;
    {
        dp_palette *p = const_cast<dp_palette *>(pal);
        std::lock_guard<std::mutex> lock(p->dev_mu);
        lut = p->dev.lut_in;
    }
    return launch_pattern(in_dev, out_dev, n_frames, h, w, y0, x0, pattern_snapshot(pal), lut, matrix, strength256, (hipStream_t)stream);
}

}  // extern "C"
