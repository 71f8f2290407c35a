// Wavelet dithering (WaveletDitherStrategy.dither, dithering_lib.py:846-941): per channel a one-level 2-D DWT (pywt.dwt2,
// mode 'symmetric', float32), each of the four subbands quantised to Q levels with uniform noise, the inverse transform
// (pywt.idwt2), crop and clip; then per pixel the nearest or the second-nearest palette entry (scipy KDTree.query(k=2)),
// chosen by a float64 uniform threshold.
//
// Per group of frames (every frame of the group in the workspace at once; frames are independent, a frame cannot be
// tiled: the subband extremes span the whole frame):
//   wl_fwd0_kernel   per (channel, axis-0 output row, column): pywt's downsampling convolution along axis 0 -> A0, D0
//   wl_fwd1_kernel   per (channel, row, axis-1 output): the same along axis 1 -> the four subbands aa, da, ad, dd
//                    (dwt2's cA, cH, cV, cD); their float32 extremes through order-preserving uint32 atomics (exact)
//   wl_inv1_kernel   per (channel, row, output column < w): subbands quantised on load, pywt's upsampling convolution
//                    along axis 1 -> Ra (from aa, ad), Rd (from da, dd), written over A0, D0
//   wl_pick_kernel   per pixel: the axis-0 inverse of Ra, Rd for each channel, clip, the two nearest entries by a float64
//                    scan of the palette (staged in LDS), the factor against the threshold, the output colour.  Points with
//                    an exact distance tie among the first three go to a list ...
//   wl_tie_kernel    ... whose pixels replay scipy's traversal (tree_query<2>: a small grid, its queue lives in scratch).
//
// Exactness.  pywt's float32 convolutions add the products tap * x in a fixed order per output that depends on where the
// output lies (left overhang, interior, filter longer than the line, right overhang: the four loops of
// downsampling_convolution); wl_dec_at runs those loops for one output.  The inverse adds sum_even / sum_odd per output into
// a zeroed row, the approximation's contribution first.  Every product and sum rounds once (__fmul_rn / __fadd_rn, no
// contraction).  The taps are pywt's float32 filters as read off its transforms with unit impulses (not all of them are
// the float32 roundings of the float64 taps: coif1's differ).
// The random stream is RandomState(seed).random_sample: the caller passes it (float64, on the device); a subband whose
// float32 min equals its max is not quantised and draws nothing, so every later offset depends on the 12 flags of the
// frame, which each thread derives from the extremes.  Thresholds follow all subband draws.
#include <cmath>

#include "dp_internal.h"
#include "tree_query.hip.h"

namespace dp {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxF = 8;
constexpr size_t kGroupBytes = 512u << 20;   // workspace of the frames that run at once (at least one frame)
constexpr size_t kHeadBytes = 256;           // per frame: 24 extreme words and the tie count, padded
constexpr int kPalLds = 1024;                // palette entries staged in LDS as float64 (24 KB)

// pywt 1.x float32 filters [wavelet][dec_lo, dec_hi, rec_lo, rec_hi][tap] (DP_WL_* order)
__constant__ float c_taps[9][4][kMaxF] = {
    // haar
    {{0x1.6a09e6p-1f, 0x1.6a09e6p-1f}, {-0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
     {0x1.6a09e6p-1f, 0x1.6a09e6p-1f}, {0x1.6a09e6p-1f, -0x1.6a09e6p-1f}},
    // db1
    {{0x1.6a09e6p-1f, 0x1.6a09e6p-1f}, {-0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
     {0x1.6a09e6p-1f, 0x1.6a09e6p-1f}, {0x1.6a09e6p-1f, -0x1.6a09e6p-1f}},
    // db2
    {{-0x1.0907dcp-3f, 0x1.cb0bf0p-3f, 0x1.ac4bdep-1f, 0x1.ee8dd4p-2f},
     {-0x1.ee8dd4p-2f, 0x1.ac4bdep-1f, -0x1.cb0bf0p-3f, -0x1.0907dcp-3f},
     {0x1.ee8dd4p-2f, 0x1.ac4bdep-1f, 0x1.cb0bf0p-3f, -0x1.0907dcp-3f},
     {-0x1.0907dcp-3f, -0x1.cb0bf0p-3f, 0x1.ac4bdep-1f, -0x1.ee8dd4p-2f}},
    // db4
    {{-0x1.5b4174p-7f, 0x1.0d60acp-5f, 0x1.f94e22p-6f, -0x1.7f0c1cp-3f, -0x1.ca7c70p-6f, 0x1.4302cep-1f, 0x1.6e005ep-1f,
      0x1.d7d052p-3f},
     {-0x1.d7d052p-3f, 0x1.6e005ep-1f, -0x1.4302cep-1f, -0x1.ca7c70p-6f, 0x1.7f0c1cp-3f, 0x1.f94e22p-6f, -0x1.0d60acp-5f,
      -0x1.5b4174p-7f},
     {0x1.d7d052p-3f, 0x1.6e005ep-1f, 0x1.4302cep-1f, -0x1.ca7c70p-6f, -0x1.7f0c1cp-3f, 0x1.f94e22p-6f, 0x1.0d60acp-5f,
      -0x1.5b4174p-7f},
     {-0x1.5b4174p-7f, -0x1.0d60acp-5f, 0x1.f94e22p-6f, 0x1.7f0c1cp-3f, -0x1.ca7c70p-6f, -0x1.4302cep-1f, 0x1.6e005ep-1f,
      -0x1.d7d052p-3f}},
    // sym2
    {{-0x1.0907dcp-3f, 0x1.cb0bf0p-3f, 0x1.ac4bdep-1f, 0x1.ee8dd4p-2f},
     {-0x1.ee8dd4p-2f, 0x1.ac4bdep-1f, -0x1.cb0bf0p-3f, -0x1.0907dcp-3f},
     {0x1.ee8dd4p-2f, 0x1.ac4bdep-1f, 0x1.cb0bf0p-3f, -0x1.0907dcp-3f},
     {-0x1.0907dcp-3f, -0x1.cb0bf0p-3f, 0x1.ac4bdep-1f, -0x1.ee8dd4p-2f}},
    // sym4
    {{-0x1.36561cp-4f, -0x1.e58c6ap-6f, 0x1.fd8fc0p-2f, 0x1.9b83a6p-1f, 0x1.3101a2p-2f, -0x1.96673cp-4f, -0x1.9d01bep-7f,
      0x1.07f8bep-5f},
     {-0x1.07f8bep-5f, -0x1.9d01bep-7f, 0x1.96673cp-4f, 0x1.3101a2p-2f, -0x1.9b83a6p-1f, 0x1.fd8fc0p-2f, 0x1.e58c6ap-6f,
      -0x1.36561cp-4f},
     {0x1.07f8bep-5f, -0x1.9d01bep-7f, -0x1.96673cp-4f, 0x1.3101a2p-2f, 0x1.9b83a6p-1f, 0x1.fd8fc0p-2f, -0x1.e58c6ap-6f,
      -0x1.36561cp-4f},
     {-0x1.36561cp-4f, 0x1.e58c6ap-6f, 0x1.fd8fc0p-2f, -0x1.9b83a6p-1f, 0x1.3101a2p-2f, 0x1.96673cp-4f, -0x1.9d01bep-7f,
      -0x1.07f8bep-5f}},
    // coif1
    {{-0x1.0080e2p-6f, -0x1.29e9aep-4f, 0x1.8a1a02p-2f, 0x1.b48450p-1f, 0x1.5a01d8p-2f, -0x1.29e9aep-4f},
     {0x1.29e9aep-4f, 0x1.5a01d8p-2f, -0x1.b48450p-1f, 0x1.8a1a02p-2f, 0x1.29e9aep-4f, -0x1.0080e2p-6f},
     {-0x1.29e9aep-4f, 0x1.5a01d8p-2f, 0x1.b48450p-1f, 0x1.8a1a02p-2f, -0x1.29e9aep-4f, -0x1.0080e2p-6f},
     {-0x1.0080e2p-6f, 0x1.29e9aep-4f, 0x1.8a1a02p-2f, -0x1.b48450p-1f, 0x1.5a01d8p-2f, 0x1.29e9aep-4f}},
    // bior1.3
    {{-0x1.6a09e6p-4f, 0x1.6a09e6p-4f, 0x1.6a09e6p-1f, 0x1.6a09e6p-1f, 0x1.6a09e6p-4f, -0x1.6a09e6p-4f},
     {0.0f, 0.0f, -0x1.6a09e6p-1f, 0x1.6a09e6p-1f, 0.0f, 0.0f},
     {0.0f, 0.0f, 0x1.6a09e6p-1f, 0x1.6a09e6p-1f, 0.0f, 0.0f},
     {-0x1.6a09e6p-4f, -0x1.6a09e6p-4f, 0x1.6a09e6p-1f, -0x1.6a09e6p-1f, 0x1.6a09e6p-4f, 0x1.6a09e6p-4f}},
    // bior2.2
    {{0.0f, -0x1.6a09e6p-3f, 0x1.6a09e6p-2f, 0x1.0f876cp+0f, 0x1.6a09e6p-2f, -0x1.6a09e6p-3f},
     {0.0f, 0x1.6a09e6p-2f, -0x1.6a09e6p-1f, 0x1.6a09e6p-2f, 0.0f, 0.0f},
     {0.0f, 0x1.6a09e6p-2f, 0x1.6a09e6p-1f, 0x1.6a09e6p-2f, 0.0f, 0.0f},
     {0.0f, 0x1.6a09e6p-3f, 0x1.6a09e6p-2f, -0x1.0f876cp+0f, 0x1.6a09e6p-2f, 0x1.6a09e6p-3f}},
};
constexpr int kFilterLen[9] = {2, 2, 4, 8, 4, 8, 6, 6, 6};

struct WlGeom {
    int h, w, n0, n1, F, wid;
    size_t plane0;    // n0 * w: one channel of A0 / D0 / Ra / Rd
    size_t sb;        // n0 * n1: one subband
    size_t frame_ws;  // floats of one frame: 6 planes of n0 * w, then 12 subbands
    const double *u;  // the caller's uniform stream
    float qf, top, qden;   // float32(Q), float32(Q - 1), float32(Q - 1 + 1e-9)
    double qd, topd, qdend;  // the same in float64 (Q >= 65536: numpy computes q in float64)
    int wide;
};

// order-preserving uint32 of a float32 (ascending); the minimum is kept as the maximum of the complement, so a zeroed
// word is the identity of both
__device__ __forceinline__ uint32_t wl_key(const float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float wl_unkey(const uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One output of pywt's downsampling_convolution (step 2, MODE_SYMMETRIC) at convolution index i = 2 o + 1, for the
// low- and high-pass filter at once (the same loop order): ld(k) reads input k of the line of length N.
template <class LD>
__device__ __forceinline__ void wl_dec_at(const LD &ld, const int N, const int F, const int i, const float *lo,
                                          const float *hi, float &sa, float &sd)
{
    float a = 0.0f, d = 0.0f;
    auto add = [&](const int m, const int k) {
        const float x = ld(k);
        a = __fadd_rn(a, __fmul_rn(lo[m], x));
        d = __fadd_rn(d, __fmul_rn(hi[m], x));
    };
    // the left mirror: taps j .. F-1 against input 0, 1, ..., N-1, N-1, ..., 0, 0, 1, ...
    auto left_mirror = [&](int j) {
        while (j < F) {
            for (int k = 0; k < N && j < F; ++j, ++k) add(j, k);
            for (int k = 0; k < N && j < F; ++k, ++j) add(j, N - 1 - k);
        }
    };
    if (i < F && i < N) {  // left boundary overhang
        int j = 0;
        for (; j <= i; ++j) add(j, i - j);
        left_mirror(j);
    } else if (i < N) {    // interior
        for (int j = 0; j < F; ++j) add(j, i - j);
    } else {               // i >= N: the right mirror first, tap i-N down to 0
        int j = 0;
        while (i - j >= N) {
            for (int k = 0; k < N && i - j >= N; ++j, ++k) add(i - N - j, N - 1 - k);
            for (int k = 0; k < N && i - j >= N; ++j, ++k) add(i - N - j, k);
        }
        if (i < F) {       // filter longer than the line
            for (; j <= i; ++j) add(j, i - j);
            left_mirror(j);
        } else {           // right boundary overhang
            for (; j < F; ++j) add(j, i - j);
        }
    }
    sa = a;
    sd = d;
}

// _quant_subband (dithering_lib.py:927-941) for one coefficient of a subband that is not constant, numpy 1.x semantics:
// (sub - mn) / float32(float64(scale) + 1e-9) in float32; then for Q < 65536 all float32 (q + noise, floor, clip,
// / float32(Q - 1 + 1e-9), * scale + mn), for larger Q the same in float64 (the Python int no longer fits numpy's
// value-based cast to float32) rounded to float32 at the end.
__device__ __forceinline__ float wl_quant(const WlGeom &g, const float v, const float mn, const float scale,
                                          const float den, const double u)
{
    const float norm = __fdiv_rn(__fsub_rn(v, mn), den);
    const float noise = (float)u;
    if (!g.wide) {
        float q = floorf(__fadd_rn(__fmul_rn(norm, g.qf), noise));
        q = q > 0.0f ? q : 0.0f;
        q = q < g.top ? q : g.top;
        return __fadd_rn(__fmul_rn(__fdiv_rn(q, g.qden), scale), mn);
    }
    double q = floor(__dadd_rn(__dmul_rn((double)norm, g.qd), (double)noise));
    q = q > 0.0 ? q : 0.0;
    q = q < g.topd ? q : g.topd;
    return (float)__dadd_rn(__dmul_rn(__ddiv_rn(q, g.qdend), (double)scale), (double)mn);
}

// one subband s (channel * 4 + aa / da / ad / dd) of a frame: its extremes, whether it draws, and its stream offset
// (subbands draw in the order of s, a constant one draws nothing)
struct WlBand {
    float mn, scale, den;
    bool draw;
    size_t off;
};

__device__ __forceinline__ bool wl_draws(const uint32_t *__restrict__ head, const int s)
{
    return !(wl_unkey(head[2 * s + 1]) == wl_unkey(~head[2 * s]));
}

__device__ __forceinline__ WlBand wl_band(const WlGeom &g, const uint32_t *__restrict__ head, const int s)
{
    WlBand b;
    int before = 0;
    for (int t = 0; t < s; ++t) before += wl_draws(head, t);
    const float mn = wl_unkey(~head[2 * s]), mx = wl_unkey(head[2 * s + 1]);
    b.draw = !(mx == mn);
    b.mn = mn;
    b.scale = __fsub_rn(mx, mn);
    b.den = (float)__dadd_rn((double)b.scale, 1e-9);
    b.off = (size_t)before * g.sb;
    return b;
}

// where the thresholds start: after every subband draw of the frame
__device__ __forceinline__ size_t wl_thr_off(const WlGeom &g, const uint32_t *__restrict__ head)
{
    int n = 0;
#pragma unroll
    for (int t = 0; t < 12; ++t) n += wl_draws(head, t);
    return (size_t)n * g.sb;
}

__device__ __forceinline__ float wl_lut(const uint8_t v, const uint8_t *__restrict__ lut) { return (float)(lut ? lut[v] : v); }

// frame layout in the workspace: [head: kHeadBytes][6 planes n0 x w: A0/Ra of channels 0-2, D0/Rd of channels 0-2]
// [12 subbands n0 x n1: channel-major, aa da ad dd]
__device__ __forceinline__ float *wl_frame(uint8_t *ws, const WlGeom &g, const unsigned f)
{
    return reinterpret_cast<float *>(ws + (size_t)f * (kHeadBytes + g.frame_ws * 4) + kHeadBytes);
}
__device__ __forceinline__ uint32_t *wl_head(uint8_t *ws, const WlGeom &g, const unsigned f)
{
    return reinterpret_cast<uint32_t *>(ws + (size_t)f * (kHeadBytes + g.frame_ws * 4));
}

__device__ __forceinline__ uint32_t *wl_ties(uint8_t *ws, const WlGeom &g, const unsigned f)
{
    return reinterpret_cast<uint32_t *>(wl_frame(ws, g, f) + 6 * g.plane0 + 12 * g.sb);
}

// grid (blocks over n0 * w, frames of the group * 3): axis 0, A0 / D0 [ch][o][x]
__global__ __launch_bounds__(kBlock) void wl_fwd0_kernel(const uint8_t *__restrict__ in, uint8_t *ws, const WlGeom g,
                                                         const uint8_t *__restrict__ lut)
{
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.plane0) return;
    const unsigned f = blockIdx.y / 3u, ch = blockIdx.y % 3u;
    const int o = (int)(p / (unsigned)g.w), x = (int)(p - (size_t)o * (unsigned)g.w);
    const uint8_t *col = in + ((size_t)f * g.h * g.w + x) * 3 + ch;
    const size_t stride = (size_t)g.w * 3;
    float a, d;
    wl_dec_at([&](const int k) { return wl_lut(col[(size_t)k * stride], lut); }, g.h, g.F, 2 * o + 1, c_taps[g.wid][0],
              c_taps[g.wid][1], a, d);
    float *fr = wl_frame(ws, g, f);
    fr[ch * g.plane0 + p] = a;
    fr[(3 + ch) * g.plane0 + p] = d;
}

__device__ __forceinline__ float wave_min(float v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// grid (blocks over n0 * n1, frames * 3): axis 1 of A0 (-> aa, ad) and D0 (-> da, dd), and the subband extremes
__global__ __launch_bounds__(kBlock) void wl_fwd1_kernel(uint8_t *ws, const WlGeom g)
{
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned f = blockIdx.y / 3u, ch = blockIdx.y % 3u;
    float *fr = wl_frame(ws, g, f);
    const float inf = __int_as_float(0x7f800000);
    float v[4] = {inf, inf, inf, inf}, u[4] = {-inf, -inf, -inf, -inf};
    if (p < g.sb) {
        const int r = (int)(p / (unsigned)g.n1), o = (int)(p - (size_t)r * (unsigned)g.n1);
        const float *lo = c_taps[g.wid][0], *hi = c_taps[g.wid][1];
        const float *ra = fr + ch * g.plane0 + (size_t)r * g.w, *rd = fr + (3 + ch) * g.plane0 + (size_t)r * g.w;
        float aa, ad, da, dd;
        wl_dec_at([&](const int k) { return ra[k]; }, g.w, g.F, 2 * o + 1, lo, hi, aa, ad);
        wl_dec_at([&](const int k) { return rd[k]; }, g.w, g.F, 2 * o + 1, lo, hi, da, dd);
        float *sbp = fr + 6 * g.plane0 + (size_t)ch * 4 * g.sb + p;
        const float c[4] = {aa, da, ad, dd};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sbp[s * g.sb] = c[s];
            v[s] = c[s];
            u[s] = c[s];
        }
    }
    // extremes: per wave by shuffles, per block in LDS, then one atomic per word and block -- and only when the block
    // improves on the value it reads first (every block of a frame and channel hits the same 8 words: unconditional
    // atomics serialised there, 1.8 ms of a 1080p frame).  A stale read only costs an atomic that changes nothing.
    __shared__ uint32_t part[kBlock / 64][8];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        // fminf / fmaxf of -0 and +0 may return either: equal values, and the key of either decodes to a value that
        // compares equal to the other, so the "constant?" test and the arithmetic (x - mn, + mn) are not affected
        const float mn = wave_min(v[s]), mx = wave_max(u[s]);
        if ((threadIdx.x & 63) == 0) {   // (an all-idle wave: +inf / -inf, whose keys are the identities' neighbours)
            part[wave][2 * s] = mn <= mx ? ~wl_key(mn) : 0u;
            part[wave][2 * s + 1] = mn <= mx ? wl_key(mx) : 0u;
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        uint32_t k = 0;
        for (int wv = 0; wv < kBlock / 64; ++wv) k = part[wv][threadIdx.x] > k ? part[wv][threadIdx.x] : k;
        uint32_t *dst = wl_head(ws, g, f) + 8 * ch + threadIdx.x;
        if (k > __atomic_load_n(dst, __ATOMIC_RELAXED)) atomicMax(dst, k);
    }
}

// a coefficient of subband b (plane sub) as the inverse transform sees it
__device__ __forceinline__ float wl_coef(const WlGeom &g, const WlBand &b, const float *__restrict__ sub, const int r,
                                         const int col)
{
    const size_t k = (size_t)r * g.n1 + col;
    const float c = sub[k];
    if (!b.draw) return c;
    return wl_quant(g, c, b.mn, b.scale, b.den, g.u[b.off + k]);
}

// grid (blocks over n0 * w, frames * 3): axis-1 inverse, output columns 0 .. w-1 -> Ra, Rd [ch][r][c] over A0, D0
__global__ __launch_bounds__(kBlock) void wl_inv1_kernel(uint8_t *ws, const WlGeom g)
{
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.plane0) return;
    const unsigned f = blockIdx.y / 3u, ch = blockIdx.y % 3u;
    const uint32_t *head = wl_head(ws, g, f);
    float *fr = wl_frame(ws, g, f);
    const int r = (int)(p / (unsigned)g.w), c = (int)(p - (size_t)r * (unsigned)g.w);
    const int e = c & 1, i = g.F / 2 - 1 + (c >> 1);
    const float *lo = c_taps[g.wid][2], *hi = c_taps[g.wid][3];
    float res[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {   // (aa, ad) -> Ra; (da, dd) -> Rd
        const int sa = 4 * ch + half, sd = 4 * ch + half + 2;
        const WlBand ba = wl_band(g, head, sa), bd = wl_band(g, head, sd);
        const float *pa = fr + 6 * g.plane0 + sa * g.sb, *pd = fr + 6 * g.plane0 + sd * g.sb;
        float A = 0.0f, D = 0.0f;
        for (int j = 0; j < g.F / 2; ++j) {
            A = __fadd_rn(A, __fmul_rn(lo[2 * j + e], wl_coef(g, ba, pa, r, i - j)));
            D = __fadd_rn(D, __fmul_rn(hi[2 * j + e], wl_coef(g, bd, pd, r, i - j)));
        }
        res[half] = __fadd_rn(__fadd_rn(0.0f, A), D);
    }
    fr[ch * g.plane0 + p] = res[0];
    fr[(3 + ch) * g.plane0 + p] = res[1];
}

// the reconstructed, cropped and clipped float32 value of pixel (y, x), channel ch: axis-0 inverse of Ra, Rd
__device__ __forceinline__ float wl_pixel(const WlGeom &g, const float *__restrict__ fr, const int ch, const int y,
                                          const int x)
{
    const int e = y & 1, i = g.F / 2 - 1 + (y >> 1);
    const float *lo = c_taps[g.wid][2], *hi = c_taps[g.wid][3];
    const float *ra = fr + ch * g.plane0 + x, *rd = fr + (3 + ch) * g.plane0 + x;
    float A = 0.0f, D = 0.0f;
    for (int j = 0; j < g.F / 2; ++j) {
        A = __fadd_rn(A, __fmul_rn(lo[2 * j + e], ra[(size_t)(i - j) * g.w]));
        D = __fadd_rn(D, __fmul_rn(hi[2 * j + e], rd[(size_t)(i - j) * g.w]));
    }
    float v = __fadd_rn(__fadd_rn(0.0f, A), D);
    v = v > 0.0f ? v : 0.0f;   // np.clip(rec, 0, 255)
    return v < 255.0f ? v : 255.0f;
}

// dithering_lib.py:915-924 with the float64 threshold: factor from the re-squared sqrt distances
__device__ __forceinline__ bool wl_use_nearest(const double d2_0, const double d2_1, const double t)
{
    const double r0 = __dsqrt_rn(d2_0), r1 = __dsqrt_rn(d2_1);
    const double s0 = __dmul_rn(r0, r0), s1 = __dmul_rn(r1, r1);
    const double tot = __dadd_rn(s0, s1);
    const double fac = (tot == 0.0) ? 0.0 : __ddiv_rn(s0, tot);
    return fac <= t;
}

__device__ __forceinline__ void wl_store(uint8_t *__restrict__ o, const uint32_t rgb)
{
    o[0] = (uint8_t)rgb;
    o[1] = (uint8_t)(rgb >> 8);
    o[2] = (uint8_t)(rgb >> 16);
}

// grid (blocks over h * w, frames of the group)
__global__ __launch_bounds__(kBlock) void wl_pick_kernel(uint8_t *ws, uint8_t *__restrict__ out, const WlGeom g,
                                                         const PalDev pal)
{
    __shared__ double sp[kPalLds * 3];
    const int K = pal.K;
    const bool staged = K <= kPalLds;
    if (staged)
        for (int j = threadIdx.x; j < 3 * K; j += kBlock) sp[j] = pal.pts[j];
    __syncthreads();
    const size_t npx = (size_t)g.h * (size_t)g.w;
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= npx) return;
    const unsigned f = blockIdx.y;
    const int y = (int)(p / (unsigned)g.w), x = (int)(p - (size_t)y * (unsigned)g.w);
    const float *fr = wl_frame(ws, g, f);
    const double x0 = wl_pixel(g, fr, 0, y, x), x1 = wl_pixel(g, fr, 1, y, x), x2 = wl_pixel(g, fr, 2, y, x);
    const double *pts = staged ? sp : pal.pts;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double b0 = inf, b1 = inf, b2 = inf;
    int i0 = K, i1 = K;
    for (int j = 0; j < K; ++j) {
        const double d = sq_dist3(pts + 3 * j, x0, x1, x2);
        if (d < b0) {
            b2 = b1;
            b1 = b0;
            i1 = i0;
            b0 = d;
            i0 = j;
        } else if (d < b1) {
            b2 = b1;
            b1 = d;
            i1 = j;
        } else if (d < b2) {
            b2 = d;
        }
    }
    uint32_t *head = wl_head(ws, g, f);
    if (b0 == b1 || (b1 == b2 && b2 != inf)) {   // which entry scipy reports first / second depends on its traversal
        wl_ties(ws, g, f)[atomicAdd(head + 24, 1u)] = (uint32_t)p;
        return;
    }
    // (a palette of one entry has no second: scipy reports index K at distance inf, the factor is 0)
    const int k = wl_use_nearest(b0, b1, g.u[wl_thr_off(g, head) + p]) ? i0 : i1;
    wl_store(out + ((size_t)f * npx + p) * 3, pal.out_rgb[k < K ? k : i0]);
}

template <int CAP>
__global__ __launch_bounds__(64) void wl_tie_kernel(uint8_t *ws, uint8_t *__restrict__ out, const WlGeom g,
                                                    const PalDev pal)
{
    const unsigned f = blockIdx.y;
    const uint32_t *head = wl_head(ws, g, f);
    const uint32_t n = head[24];
    const uint32_t *ties = wl_ties(ws, g, f);
    const float *fr = wl_frame(ws, g, f);
    const size_t npx = (size_t)g.h * (size_t)g.w;
    for (uint32_t t = blockIdx.x * 64u + threadIdx.x; t < n; t += gridDim.x * 64u) {
        const uint32_t p = ties[t];
        const int y = (int)(p / (unsigned)g.w), x = (int)(p - (uint32_t)y * (unsigned)g.w);
        double d2[2];
        int ii[2];
        tree_query<2, CAP>(pal, wl_pixel(g, fr, 0, y, x), wl_pixel(g, fr, 1, y, x), wl_pixel(g, fr, 2, y, x), d2, ii);
        const int k = wl_use_nearest(d2[0], d2[1], g.u[wl_thr_off(g, head) + p]) ? ii[0] : ii[1];
        wl_store(out + ((size_t)f * npx + p) * 3, pal.out_rgb[k < pal.K ? k : ii[0]]);
    }
}

// subband side and the floats of one frame's workspace
static void wl_shape(int h, int w, int F, int &n0, int &n1, size_t &frame_floats)
{
    n0 = (h + F - 1) / 2;
    n1 = (w + F - 1) / 2;
    frame_floats = 6 * (size_t)n0 * w + 12 * (size_t)n0 * n1 + (size_t)h * w;
}

static int64_t wl_group(int64_t n_frames, size_t per_frame)
{
    int64_t g = (int64_t)(kGroupBytes / per_frame);
    if (g < 1) g = 1;
    if (g > 65535 / 3) g = 65535 / 3;
    return g < n_frames ? g : n_frames;
}

}  // namespace

int wavelet_filter_len(int wid) { return (wid >= 0 && wid < 9) ? kFilterLen[wid] : 0; }

int64_t wavelet_uniforms_needed(int h, int w, int wid)
{
    int n0, n1;
    size_t ff;
    wl_shape(h, w, kFilterLen[wid], n0, n1, ff);
    return 12 * (int64_t)n0 * n1 + (int64_t)h * w;
}

size_t wavelet_ws_bytes(int64_t n_frames, int h, int w, int wid)
{
    int n0, n1;
    size_t ff;
    wl_shape(h, w, kFilterLen[wid], n0, n1, ff);
    const size_t per = kHeadBytes + ff * 4;
    return (size_t)wl_group(n_frames, per) * per;
}

int launch_wavelet(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, const PalDev &pal,
                   const dp_wavelet_params &P, void *ws, size_t ws_bytes, hipStream_t s)
{
    WlGeom g;
    size_t ff;
    g.h = h;
    g.w = w;
    g.wid = P.wavelet;
    g.F = kFilterLen[P.wavelet];
    wl_shape(h, w, g.F, g.n0, g.n1, ff);
    g.plane0 = (size_t)g.n0 * w;
    g.sb = (size_t)g.n0 * g.n1;
    g.frame_ws = ff;
    g.u = P.uniforms_dev;
    const int Q = P.subband_quant;
    g.qf = (float)Q;
    g.top = (float)(Q - 1);
    g.qden = (float)((double)(Q - 1) + 1e-9);
    g.qd = (double)Q;
    g.topd = (double)(Q - 1);
    g.qdend = (double)(Q - 1) + 1e-9;
    g.wide = Q >= 65536;
    const size_t per = kHeadBytes + ff * 4;
    const int64_t G = wl_group(n_frames, per);
    if (ws_bytes < (size_t)G * per) {
        set_error("dp_wavelet_u8: workspace too small (see dp_wavelet_workspace_bytes)");
        return DP_EWORKSPACE;
    }
    uint8_t *wsb = static_cast<uint8_t *>(ws);
    const size_t npx = (size_t)h * (size_t)w;
    const unsigned b0 = (unsigned)((g.plane0 + kBlock - 1) / kBlock), b1 = (unsigned)((g.sb + kBlock - 1) / kBlock),
                   bp = (unsigned)((npx + kBlock - 1) / kBlock);
    const bool big = pal.n_inner > kQueueSmall;
    ProfMark *pm = prof_begin(s);
    for (int64_t f0 = 0; f0 < n_frames; f0 += G) {
        const unsigned gn = (unsigned)(n_frames - f0 < G ? n_frames - f0 : G);
        const uint8_t *fin = in + (size_t)f0 * npx * 3;
        uint8_t *fout = out + (size_t)f0 * npx * 3;
        for (unsigned f = 0; f < gn; ++f) DP_HIP(hipMemsetAsync(wsb + (size_t)f * per, 0, kHeadBytes, s));
        hipLaunchKernelGGL(wl_fwd0_kernel, dim3(b0, gn * 3), dim3(kBlock), 0, s, fin, wsb, g, pal.lut_in);
        hipLaunchKernelGGL(wl_fwd1_kernel, dim3(b1, gn * 3), dim3(kBlock), 0, s, wsb, g);
        hipLaunchKernelGGL(wl_inv1_kernel, dim3(b0, gn * 3), dim3(kBlock), 0, s, wsb, g);
        hipLaunchKernelGGL(wl_pick_kernel, dim3(bp, gn), dim3(kBlock), 0, s, wsb, fout, g, pal);
        if (big)
            hipLaunchKernelGGL(wl_tie_kernel<kQueueLarge>, dim3(64, gn), dim3(64), 0, s, wsb, fout, g, pal);
        else
            hipLaunchKernelGGL(wl_tie_kernel<kQueueSmall>, dim3(64, gn), dim3(64), 0, s, wsb, fout, g, pal);
    }
    prof_end(pm, s);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

}  // namespace dp
