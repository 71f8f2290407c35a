// The Oklab colour metric (include/ditherpie_hip_metric.h): palettes whose nearest entry is measured in an integer Oklab.
//
// A metric palette is searched only through an exact table of (nearest, second) over all 2^24 colours, two bytes per colour in
// the brick order of the pattern table (pattern_tab.hip.h: 4 x 4 x 4 colours per line, here 128 bytes), built by brute force:
//
// metric_build_kernel    one lane owns 8 consecutive table addresses (one 16-byte store); the palette's Lab records in LDS, every
//                        lane reads the same entry (a broadcast); entries in ascending order under strict comparisons, so an
//                        equal distance never displaces a lower index: the pair order of the definition, exact by construction
// metric_rank_kernel     the pattern / dot-diffusion table of a metric palette: rank_of[nearest] of 4 addresses, one dword store
// metric_ordered_kernel  four pixels per lane (12 bytes), one gather per pixel; DP_MODE_NEAREST is the gather alone,
//                        DP_MODE_MATRIX also computes the pixel's Lab, the two distances and the float64 decision
// metric_lab_kernel      (L, a, b) of packed RGB pixels, by the device function the kernels above use
//
// The cube root floor(cbrt(x * 2^32)), x < 2^16: v_log_f32 / v_exp_f32 give an estimate within a tenth of a unit, one step down
// and one step up against the 48-bit cube (two 32-bit multiplies and a mul_hi each) make it exact.  The alternative, a gather
// from a 65536-entry table in global memory, is compiled into the experiments build (DP_METRIC_CBRT_TABLE=1 when the table is
// built) so that the A/B can be repeated: DESIGN.md 4.3h has both timings.
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_metric.h"
#include "metric_lab.hip.h"
#include "pattern_tab.hip.h"

namespace dp {
namespace {

constexpr int kMetBlock = 256;
constexpr size_t kMetTabBytes = (size_t)DP_METRIC_TABLE_BYTES;
constexpr size_t kMetSideBytes = 256 * sizeof(int4) + 256 * sizeof(uint32_t);   // lab, out_rgb
constexpr size_t kCbrtBytes = 65536 * sizeof(uint16_t);
constexpr uint32_t kBuildPerLane = 8;

// tab8[t] = nearest | second << 8 of table addresses 8 t .. 8 t + 7; the grid covers 2^24 / 8 lanes exactly.  md.K >= 2
template <bool TAB>
__global__ __launch_bounds__(kMetBlock) void metric_build_kernel(uint4 *__restrict__ tab8, const MetDev md)
{
    __shared__ int4 s_lab[256];
    __shared__ uint16_t s_lin[256];
    for (int i = threadIdx.x; i < 256; i += kMetBlock) {
        s_lab[i] = md.lab[i];
        s_lin[i] = c_lin[i];
    }
    __syncthreads();
    const uint32_t t = blockIdx.x * kMetBlock + threadIdx.x;
    const uint32_t a0 = t * kBuildPerLane;
    int L[kBuildPerLane], A[kBuildPerLane], B[kBuildPerLane], d0[kBuildPerLane], d1[kBuildPerLane];
    uint32_t i0[kBuildPerLane], i1[kBuildPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kBuildPerLane; ++j) {
        const uint32_t c = tab_colour<true>(a0 + j);
        lab_dev<TAB>(c & 255u, (c >> 8) & 255u, c >> 16, s_lin, md.cbrt, L[j], A[j], B[j]);
        d0[j] = d1[j] = 0x7fffffff;
        i0[j] = i1[j] = 0u;
    }
    for (int k = 0; k < md.K; ++k) {
        const int4 e = s_lab[k];
#pragma unroll
        for (uint32_t j = 0; j < kBuildPerLane; ++j) {
            const int x = L[j] - e.x, y = A[j] - e.y, z = B[j] - e.z;   // |.| < 2^15: 24-bit products
            const int d = __mul24(x, x) + __mul24(y, y) + __mul24(z, z);
            const bool first = d < d0[j], second = d < d1[j];
            d1[j] = first ? d0[j] : (second ? d : d1[j]);
            i1[j] = first ? i0[j] : (second ? (uint32_t)k : i1[j]);
            d0[j] = first ? d : d0[j];
            i0[j] = first ? (uint32_t)k : i0[j];
        }
    }
    uint32_t w[kBuildPerLane / 2];
#pragma unroll
    for (uint32_t j = 0; j < kBuildPerLane; j += 2) w[j / 2] = i0[j] | (i1[j] << 8) | (i0[j + 1] << 16) | (i1[j + 1] << 24);
    tab8[t] = make_uint4(w[0], w[1], w[2], w[3]);
}

// out4[t] = rank_of[nearest] of table addresses 4 t .. 4 t + 3; the grid covers 2^24 / 4 lanes exactly
__global__ __launch_bounds__(kMetBlock) void metric_rank_kernel(const uint2 *__restrict__ tab4, const uint32_t *__restrict__ rank_of,
                                                                uint32_t *__restrict__ out4)
{
    __shared__ uint32_t s_rank[256];
    for (int i = threadIdx.x; i < 256; i += kMetBlock) s_rank[i] = rank_of[i];
    __syncthreads();
    const uint32_t t = blockIdx.x * kMetBlock + threadIdx.x;
    const uint2 v = tab4[t];
    out4[t] = s_rank[v.x & 255u] | (s_rank[(v.x >> 16) & 255u] << 8) | (s_rank[v.y & 255u] << 16) | (s_rank[(v.y >> 16) & 255u] << 24);
}

// in and out may be the same buffer (no __restrict__): a lane reads its four pixels before it writes them.  `aligned`: both
// buffers and every frame of them start on a dword
template <bool MATRIX, bool TAB>
__global__ __launch_bounds__(kMetBlock) void metric_ordered_kernel(const uint8_t *in, uint8_t *out, const uint32_t hw, const uint32_t w,
                                                                   const uint32_t y0, const uint32_t x0, const int aligned, const MetDev md,
                                                                   const float *__restrict__ thr, const uint32_t th_h, const uint32_t th_w)
{
    __shared__ uint32_t s_out[256];
    __shared__ int4 s_lab[MATRIX ? 256 : 1];
    __shared__ uint16_t s_lin[MATRIX ? 256 : 1];
    for (int i = threadIdx.x; i < 256; i += kMetBlock) {
        s_out[i] = md.out_rgb[i];
        if (MATRIX) {
            s_lab[i] = md.lab[i];
            s_lin[i] = c_lin[i];
        }
    }
    __syncthreads();

    const uint32_t p0 = (blockIdx.x * kMetBlock + threadIdx.x) * 4u;
    if (p0 >= hw) return;
    const size_t fbase = (size_t)blockIdx.y * 3u * (size_t)hw;
    const uint8_t *fin = in + fbase;
    uint8_t *fout = out + fbase;
    const bool whole = aligned && p0 + 4u <= hw;
    uint32_t px[4];
    if (whole) {
        const uint32_t *in32 = reinterpret_cast<const uint32_t *>(fin) + (size_t)(p0 / 4u) * 3u;
        const uint32_t w0 = in32[0], w1 = in32[1], w2 = in32[2];
        px[0] = w0 & 0xffffffu;
        px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
        px[3] = w2 >> 8;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            px[q] = 0u;
            if (p0 + q < hw) {
                const uint8_t *s = fin + (size_t)(p0 + q) * 3u;
                px[q] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
            }
        }
    }
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = md.tab[tab_addr<true>(px[q] & 255u, (px[q] >> 8) & 255u, px[q] >> 16)];   // < 2^24: in the table

    uint32_t c[4];
    if (!MATRIX) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = s_out[v[q] & 255u];
    } else {
        uint32_t y = p0 / w, x = p0 - y * w;
        uint32_t ty = (y0 + y) % th_h, tx = (x0 + x) % th_w;
        const uint32_t tx_row = x0 % th_w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double t = (double)thr[ty * th_w + tx];
            uint32_t k = v[q] & 255u;
            // d0 <= d1, so d0 / (d0 + d1) <= 1/2 exactly and its rounded quotient is <= 0.5 too: a threshold of 0.5 or more always
            // takes nearest.  On a Bayer matrix the lanes of a wave agree on that per slot q (columns x and x + 4 lie on the same
            // side of 1/2), so half the slots skip the Lab, the distances and the division as a wave.
            if (!(t >= 0.5)) {   // (a NaN threshold goes through the division, as in the statement)
                int L, A, B;
                lab_dev<TAB>(px[q] & 255u, (px[q] >> 8) & 255u, px[q] >> 16, s_lin, md.cbrt, L, A, B);
                const uint32_t k1 = v[q] >> 8;
                const int4 e0 = s_lab[k], e1 = s_lab[k1];
                const int ax = L - e0.x, ay = A - e0.y, az = B - e0.z, bx = L - e1.x, by = A - e1.y, bz = B - e1.z;
                const int d0 = __mul24(ax, ax) + __mul24(ay, ay) + __mul24(az, az), d1 = __mul24(bx, bx) + __mul24(by, by) + __mul24(bz, bz);
                const double s = (double)d0 + (double)d1;
                const double f = s > 0.0 ? (double)d0 / s : 0.0;   // IEEE float64 division: the definition
                if (!(f <= t)) k = k1;
            }
            c[q] = s_out[k];
            ++x;
            if (++tx == th_w) tx = 0u;
            if (x == w) {
                x = 0u;
                tx = tx_row;
                if (++ty == th_h) ty = 0u;
            }
        }
    }
    if (whole) {
        uint32_t *o32 = reinterpret_cast<uint32_t *>(fout) + (size_t)(p0 / 4u) * 3u;
        o32[0] = c[0] | (c[1] << 24);
        o32[1] = (c[1] >> 8) | (c[2] << 16);
        o32[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (p0 + q < hw) {
                uint8_t *o = fout + (size_t)(p0 + q) * 3u;
                o[0] = (uint8_t)c[q];
                o[1] = (uint8_t)(c[q] >> 8);
                o[2] = (uint8_t)(c[q] >> 16);
            }
    }
}

__global__ __launch_bounds__(kMetBlock) void metric_lab_kernel(const uint8_t *__restrict__ in, int32_t *__restrict__ lab, const uint32_t n)
{
    __shared__ uint16_t s_lin[256];
    for (int i = threadIdx.x; i < 256; i += kMetBlock) s_lin[i] = c_lin[i];
    __syncthreads();
    const uint32_t p = blockIdx.x * kMetBlock + threadIdx.x;
    if (p >= n) return;
    const uint8_t *s = in + (size_t)p * 3u;
    int L, A, B;
    lab_dev<false>(s[0], s[1], s[2], s_lin, nullptr, L, A, B);
    int32_t *o = lab + (size_t)p * 3u;
    o[0] = L;
    o[1] = A;
    o[2] = B;
}

template <bool MATRIX>
void launch_metric_ordered_m(const dim3 grid, const uint8_t *in, uint8_t *out, uint32_t hw, uint32_t w, uint32_t y0, uint32_t x0, int aligned,
                             const MetDev &md, const ThrDev *thr, hipStream_t s)
{
    const float *t = MATRIX ? thr->f32 : nullptr;
    const uint32_t th_h = MATRIX ? (uint32_t)thr->th_h : 1u, th_w = MATRIX ? (uint32_t)thr->th_w : 1u;
#ifdef DP_EXPERIMENTS
    if (md.cbrt) {
        hipLaunchKernelGGL((metric_ordered_kernel<MATRIX, true>), grid, dim3(kMetBlock), 0, s, in, out, hw, w, y0, x0, aligned, md, t, th_h, th_w);
        return;
    }
#endif
    hipLaunchKernelGGL((metric_ordered_kernel<MATRIX, false>), grid, dim3(kMetBlock), 0, s, in, out, hw, w, y0, x0, aligned, md, t, th_h, th_w);
}

int launch_metric_ordered(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, int y0, int x0, const MetDev &md, int mode,
                          const ThrDev *thr, hipStream_t s)
{
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    // the 12-byte form needs every frame on a dword: always with one frame, otherwise when a frame is a multiple of 4 bytes
    const int aligned = ((((uintptr_t)in | (uintptr_t)out) & 3) == 0 && (n_frames == 1 || (3ull * hw) % 4 == 0)) ? 1 : 0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const uint32_t nf = (uint32_t)std::min<int64_t>(65535, n_frames - f0);
        const uint8_t *in_c = in + (size_t)f0 * hw * 3;
        uint8_t *out_c = out + (size_t)f0 * hw * 3;
        const dim3 grid((hw + kMetBlock * 4 - 1) / (kMetBlock * 4), nf);
        ProfMark *pm = prof_begin(s);
        if (mode == DP_MODE_MATRIX) launch_metric_ordered_m<true>(grid, in_c, out_c, hw, (uint32_t)w, (uint32_t)y0, (uint32_t)x0, aligned, md, thr, s);
        else launch_metric_ordered_m<false>(grid, in_c, out_c, hw, (uint32_t)w, (uint32_t)y0, (uint32_t)x0, aligned, md, thr, s);
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

MetDev metric_snapshot(const dp_palette *pal_c)
{
    dp_palette *p = const_cast<dp_palette *>(pal_c);
    std::lock_guard<std::mutex> lock(p->dev_mu);
    return p->met;
}

int metric_ensure_table(const dp_palette *pal_c, hipStream_t s)
{
    dp_palette *p = const_cast<dp_palette *>(pal_c);
    std::lock_guard<std::mutex> lock(p->build_mu);
    return metric_ensure_table_locked(p, s);
}

}  // namespace

bool metric_refused(const char *fn, const dp_palette *pal)
{
    if (!pal || pal->metric == DP_METRIC_RGB) return false;
    set_error("%s: the palette was created with the Oklab metric, which this entry point does not support (it searches in RGB)", fn);
    return true;
}

// Build the table once (the caller holds build_mu; the launch goes to `s`, which is waited for before the table is published:
// another thread may use it on another stream at once).  A failed build leaves the palette without a table; the next call retries.
int metric_ensure_table_locked(dp_palette *p, hipStream_t s)
{
    if (p->met.tab) return DP_OK;
    const int K = p->dev.K;
    std::vector<float> pal((size_t)3 * K);
    for (int i = 0; i < 3 * K; ++i) pal[i] = (float)p->pts_host[i];
    std::vector<int32_t> coords((size_t)3 * K);
    metric_palette_coords(pal.data(), K, 1, coords.data());
    std::vector<uint32_t> side(kMetSideBytes / sizeof(uint32_t), 0u);   // int4 lab[256] | uint32 out_rgb[256]
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < 3; ++c) side[4 * k + c] = (uint32_t)coords[3 * k + c];
    const uint32_t *out_rgb;
    {
        std::lock_guard<std::mutex> dl(p->dev_mu);
        out_rgb = p->dev.out_rgb;
    }
    DP_HIP(hipMemcpy(side.data() + 1024, out_rgb, sizeof(uint32_t) * K, hipMemcpyDeviceToHost));
    const bool cbrt_tab = exp_env("DP_METRIC_CBRT_TABLE") != nullptr;
    void *blob = nullptr;
    DP_HIP(hipMalloc(&blob, kMetTabBytes + kMetSideBytes + (cbrt_tab ? kCbrtBytes : 0)));
    uint8_t *base = reinterpret_cast<uint8_t *>(blob);
    hipError_t e = hipMemcpy(base + kMetTabBytes, side.data(), kMetSideBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && cbrt_tab) e = hipMemcpy(base + kMetTabBytes + kMetSideBytes, metric_cbrt_table(), kCbrtBytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? DP_OK : hip_fail(e, "metric table upload");
    const MetDev md{reinterpret_cast<const uint16_t *>(base), reinterpret_cast<const int4 *>(base + kMetTabBytes),
                    reinterpret_cast<const uint32_t *>(base + kMetTabBytes + 256 * sizeof(int4)),
                    cbrt_tab ? reinterpret_cast<const uint16_t *>(base + kMetTabBytes + kMetSideBytes) : nullptr, K};
    if (rc == DP_OK) {
        if (K == 1) {   // nearest = second = entry 0
            e = hipMemsetAsync(base, 0, kMetTabBytes, s);
            if (e != hipSuccess) rc = hip_fail(e, "metric table memset");
        } else {
            const dim3 grid((uint32_t)((kMetTabBytes / 2) / kBuildPerLane / kMetBlock));
            ProfMark *pm = prof_begin(s);
#ifdef DP_EXPERIMENTS
            if (cbrt_tab) hipLaunchKernelGGL(metric_build_kernel<true>, grid, dim3(kMetBlock), 0, s, reinterpret_cast<uint4 *>(base), md);
            else
#endif
                hipLaunchKernelGGL(metric_build_kernel<false>, grid, dim3(kMetBlock), 0, s, reinterpret_cast<uint4 *>(base), md);
            prof_end(pm, s);
            e = hipGetLastError();
            if (e != hipSuccess) rc = hip_fail(e, "metric table launch");
        }
    }
    if (rc == DP_OK) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "metric table build");
    }
    if (rc != DP_OK) {
        (void)hipFree(blob);
        return rc;
    }
    p->met_blob = blob;
    std::lock_guard<std::mutex> dl(p->dev_mu);
    p->met = md;
    return DP_OK;
}

int launch_metric_rank_table(const MetDev &md, const uint32_t *rank_of, uint8_t *tab, hipStream_t s)
{
    const dim3 grid((uint32_t)((kMetTabBytes / 2) / 4 / kMetBlock));
    hipLaunchKernelGGL(metric_rank_kernel, grid, dim3(kMetBlock), 0, s, reinterpret_cast<const uint2 *>(md.tab), rank_of,
                       reinterpret_cast<uint32_t *>(tab));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DP_OK : hip_fail(e, "metric rank table launch");
}

}  // namespace dp

using namespace dp;

extern "C" {

int dp_palette_create_metric(const float *pal_f32, const uint8_t *out_colors, int K, int metric, dp_palette **out)
{
    if (metric != DP_METRIC_RGB && metric != DP_METRIC_OKLAB) {
        set_error("dp_palette_create_metric: unknown metric %d", metric);
        return DP_EINVAL;
    }
    if (metric == DP_METRIC_OKLAB && pal_f32 && out_colors && out && K >= 1 && !metric_palette_ok(pal_f32, K)) {
        set_error("dp_palette_create_metric: the Oklab metric needs at most 256 colours and integer palette values in [0, 255]");
        return DP_EUNSUPPORTED;
    }
    return palette_create_impl("dp_palette_create_metric", pal_f32, out_colors, K, nullptr, metric, out);
}

int dp_palette_metric(const dp_palette *pal) { return pal ? pal->metric : -1; }

size_t dp_metric_table_bytes(const dp_palette *pal)
{
    return pal && pal->metric == DP_METRIC_OKLAB ? kMetTabBytes + kMetSideBytes : 0;
}

int dp_metric_prepare(dp_palette *pal)
{
    if (!pal || pal->metric != DP_METRIC_OKLAB) {
        set_error("dp_metric_prepare: bad argument (NULL palette, or one without a metric: use dp_palette_create_metric)");
        return DP_EINVAL;
    }
    return metric_ensure_table(pal, nullptr);
}

int dp_metric_ordered_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, int y0, int x0, const dp_palette *pal,
                         int mode, const dp_thresholds *thr, void *stream)
{
    const bool sizes_ok = n_frames >= 0 && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)h * w <= (int64_t)1 << 30 &&
                          (int64_t)y0 + h <= (int64_t)1 << 30 && (int64_t)x0 + w <= (int64_t)1 << 30;
    if (!pal || !sizes_ok || (n_frames > 0 && (!in_dev || !out_dev))) {
        set_error("dp_metric_ordered_u8: bad argument (pointers, n_frames >= 0, h, w >= 1, h * w <= 2^30, y0, x0 >= 0)");
        return DP_EINVAL;
    }
    if (mode == DP_MODE_IGN) {
        set_error("dp_metric_ordered_u8: interleaved gradient noise is not supported under a metric");
        return DP_EUNSUPPORTED;
    }
    if (mode != DP_MODE_NEAREST && mode != DP_MODE_MATRIX) {
        set_error("dp_metric_ordered_u8: unknown mode %d", mode);
        return DP_EINVAL;
    }
    if (mode == DP_MODE_MATRIX && !thr) {
        set_error("dp_metric_ordered_u8: the matrix mode needs a threshold matrix");
        return DP_EINVAL;
    }
    if (pal->metric != DP_METRIC_OKLAB) {
        set_error("dp_metric_ordered_u8: the palette has no metric (use dp_palette_create_metric, or dp_ordered_u8)");
        return DP_EINVAL;
    }
    if (n_frames == 0) return DP_OK;
    const int rc = metric_ensure_table(pal, (hipStream_t)stream);
    if (rc != DP_OK) return rc;
    return launch_metric_ordered(in_dev, out_dev, n_frames, h, w, y0, x0, metric_snapshot(pal), mode, thr ? &thr->dev : nullptr,
                                 (hipStream_t)stream);
}

int dp_metric_lab_u8(const uint8_t *in_dev, int32_t *lab_dev, int64_t n_px, void *stream)
{
    if (n_px < 0 || n_px > 0x7fffffff || (n_px > 0 && (!in_dev || !lab_dev)) || ((uintptr_t)lab_dev & 3)) {
        set_error("dp_metric_lab_u8: bad argument (pointers, 0 <= n_px <= 2^31 - 1, lab_dev 4-byte aligned)");
        return DP_EINVAL;
    }
    if (n_px == 0) return DP_OK;
    const dim3 grid((uint32_t)((n_px + kMetBlock - 1) / kMetBlock));
    hipLaunchKernelGGL(metric_lab_kernel, grid, dim3(kMetBlock), 0, (hipStream_t)stream, in_dev, lab_dev, (uint32_t)n_px);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int dp_metric_lab_host(const uint8_t *rgb_host, int64_t n, int32_t *lab_host)
{
    if (n < 0 || (n > 0 && (!rgb_host || !lab_host))) {
        set_error("dp_metric_lab_host: bad argument");
        return DP_EINVAL;
    }
    const uint16_t *ct = metric_cbrt_table();
    for (int64_t i = 0; i < n; ++i) metric_lab(rgb_host[3 * i], rgb_host[3 * i + 1], rgb_host[3 * i + 2], ct, lab_host + 3 * i);
    return DP_OK;
}

int dp_metric_top2_host(const uint8_t *rgb_host, int64_t n, const float *pal_f32, int K, int metric, uint8_t *idx0_host, uint8_t *idx1_host)
{
    if (n < 0 || !pal_f32 || K < 1 || (n > 0 && (!rgb_host || !idx0_host || !idx1_host)) || (metric != DP_METRIC_RGB && metric != DP_METRIC_OKLAB)) {
        set_error("dp_metric_top2_host: bad argument (pointers, n >= 0, K >= 1, a known metric)");
        return DP_EINVAL;
    }
    if (!metric_palette_ok(pal_f32, K)) {
        set_error("dp_metric_top2_host: at most 256 colours and integer palette values in [0, 255] are supported");
        return DP_EUNSUPPORTED;
    }
    std::vector<int32_t> coords((size_t)3 * K);
    metric_palette_coords(pal_f32, K, metric == DP_METRIC_OKLAB, coords.data());
    metric_top2(rgb_host, n, coords.data(), K, metric == DP_METRIC_OKLAB, idx0_host, idx1_host, nullptr, nullptr);
    return DP_OK;
}

}  // extern "C"
