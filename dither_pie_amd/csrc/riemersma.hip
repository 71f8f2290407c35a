// Riemersma dithering (RiemersmaDitherStrategy.dither, dithering_lib.py:812-841): error diffusion along a Hilbert curve.
//
// The reference walks the path of _hilbert_order(dim) (dim = _next_power_of_two(max(h, w)), :771-809), visits the indices
// that fall inside the image and pushes err * w into path indices i+1 .. i+4 (weights 7/16, 1/16, 5/16, 3/16; float32
// product, float32 add, clipped to [0, 255] after every add; targets outside the image receive nothing).  Each target
// gets its adds in source order, so the PULL form is exact: at in-image step j, start from the input value and add the
// contributions of j-4, j-3, j-2, j-1 (weights 3/16, 5/16, 1/16, 7/16) that are in the image, clipping after each.
// Only e_{j-1} is on the dependency chain.
//
// riemersma_kernel: one 64-lane wave per frame.
//   Lookahead: lanes compute the (row, col) of 64 consecutive path indices, a ballot + mbcnt compacts the in-image ones
//   into lanes 0.., and their raw pixels are loaded one block ahead of the walk.  Aligned runs of 4^L indices whose
//   2^L x 2^L square lies outside the image are skipped in one jump (L >= 3), so off-image indices cost next to nothing.
//   Walk: the last four in-image errors and their path indices live in registers; the nearest colour comes from the
//   lane-parallel palette scan of the one-wave-per-frame kernels (ed_nearest.hip.h: wave_nearest -- entry l + 64 m in lane l,
//   float32 prefilter with the margin test, nearest_f64 on near ties with scipy's traversal replay on exact ties).
#include "dp_internal.h"
#include "tree_query.hip.h"
#include "wave_util.hip.h"
#include "ed_nearest.hip.h"

namespace dp {
namespace {

// (x, y) of path index t on the Hilbert curve of a 2^bits-wide square: the reference's hilbert_xy loop (:777-794)
__device__ __forceinline__ void hilbert_xy(uint64_t t, const int bits, uint32_t &xo, uint32_t &yo)
{
    uint32_t x = 0, y = 0;
    for (int lvl = 0; lvl < bits; ++lvl) {
        const uint32_t s = 1u << lvl;
        const uint32_t rx = (uint32_t)(t >> 1) & 1u;
        const uint32_t ry = ((uint32_t)t ^ rx) & 1u;
        const uint32_t fx = (ry == 0u && rx == 1u) ? s - 1u - x : x;
        const uint32_t fy = (ry == 0u && rx == 1u) ? s - 1u - y : y;
        x = (ry == 0u ? fy : fx) + s * rx;
        y = (ry == 0u ? fx : fy) + s * ry;
        t >>= 2;
    }
    xo = x;
    yo = y;
}

__device__ __forceinline__ float rm_clamp255(const float v) { return __builtin_amdgcn_fmed3f(v, 0.0f, 255.0f); }

// weight with which path index p receives the error of path index q (d = p - q): 7/16, 1/16, 5/16, 3/16 for d = 1..4, else 0.
// Branch-free (a chain of compares compiled to a dozen scalar branches per source): the numerators are the nibbles of 0x35170.
__device__ __forceinline__ float rm_weight(const int64_t d)
{
    const uint64_t dm = (uint64_t)d - 1ull;
    const uint32_t sh = dm < 4ull ? 4u * ((uint32_t)dm + 1u) : 0u;
    return (float)((0x35170u >> sh) & 15u) * 0.0625f;
}

template <int CAP, int M>  // M: palette entries per lane (K <= 64 * M)
__global__ __launch_bounds__(64) void riemersma_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int h,
                                                       const int w, const int bits, const PalDev pal)
{
    extern __shared__ __align__(16) float4 s_pal[];  // M > 1: K x {x, y, z, out_rgb}
    __shared__ uint8_t s_lut[256];
    __shared__ uint32_t s_row[64], s_col[64], s_off[64];
    const int lane = threadIdx.x;
    const size_t npx = (size_t)h * (size_t)w;
    const uint8_t *fin = in + (size_t)blockIdx.x * npx * 3;
    uint8_t *fout = out + (size_t)blockIdx.x * npx * 3;
    const int K = pal.K;
    const uint64_t N = 1ull << (2 * bits);
    const uint32_t uh = (uint32_t)h, uw = (uint32_t)w;

    float4 pc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int j = lane + 64 * m;
        pc[m] = j < K ? pal.fcand[j] : make_float4(1e30f, 1e30f, 1e30f, 0.f);  // distance overflows to +inf
    }
    if (M > 1)
        for (int j = lane; j < K; j += 64) s_pal[j] = pal.fcand[j];
    for (int i = lane; i < 256; i += 64) s_lut[i] = pal.lut_in ? pal.lut_in[i] : (uint8_t)i;
    __syncthreads();

    // The next block of the path from t on (t a multiple of 64) that holds an in-image index: off-image squares skipped,
    // the in-image indices compacted into lanes 0 .. cnt-1 (this lane: its row, col and path index).  cnt = 0: path done.
    auto next_block = [&](uint64_t &t, int &cnt, uint32_t &row, uint32_t &col, uint64_t &pidx) {
        cnt = 0;
        row = col = 0u;
        pidx = 0ull;
        while (t < N) {
            uint32_t x, y;
            hilbert_xy(t, bits, x, y);  // (uniform)
            const int lmax = t == 0ull ? bits : min(bits, __builtin_ctzll(t) >> 1);
            int jump = 0;
            for (int L = lmax; L >= 3; --L) {  // a square outside the image holds only squares outside the image
                if (((y >> L) << L) >= uh || ((x >> L) << L) >= uw) {
                    jump = L;
                    break;
                }
            }
            if (jump) {
                t += 1ull << (2 * jump);
                continue;
            }
            const uint64_t idx = t + (uint64_t)lane;
            uint32_t lx, ly;
            hilbert_xy(idx, bits, lx, ly);
            const bool inside = idx < N && ly < uh && lx < uw;
            const unsigned long long mask = __ballot(inside);
            t += 64ull;
            if (mask == 0ull) continue;
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (inside) {
                s_row[pos] = ly;
                s_col[pos] = lx;
                s_off[pos] = (uint32_t)lane;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            cnt = __popcll(mask);
            if (lane < cnt) {
                row = s_row[lane];
                col = s_col[lane];
                pidx = t - 64ull + s_off[lane];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            return;
        }
    };
    // (lanes past cnt read pixel (0, 0): no branch around the loads, so nothing waits for them before the walk needs them)
    auto load_px = [&](const uint32_t row, const uint32_t col) -> uint32_t {
        const uint8_t *px = fin + ((size_t)row * uw + col) * 3;
        return (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    };

    uint64_t t = 0ull;
    int cnt;
    uint32_t row, col;
    uint64_t pidx;
    next_block(t, cnt, row, col, pidx);
    uint32_t raw = load_px(row, col);
    // the last four in-image steps, oldest first: path index (-8: none) and error
    int64_t q0 = -8, q1 = -8, q2 = -8, q3 = -8;
    float e0x = 0.f, e0y = 0.f, e0z = 0.f, e1x = 0.f, e1y = 0.f, e1z = 0.f;
    float e2x = 0.f, e2y = 0.f, e2z = 0.f, e3x = 0.f, e3y = 0.f, e3z = 0.f;
    while (cnt > 0) {
        int ncnt;
        uint32_t nrow, ncol;
        uint64_t npidx;
        next_block(t, ncnt, nrow, ncol, npidx);
        const uint32_t nraw = load_px(nrow, ncol);  // in flight during the walk
        const float p0 = (float)s_lut[raw & 255u], p1 = (float)s_lut[(raw >> 8) & 255u], p2 = (float)s_lut[(raw >> 16) & 255u];
        const uint32_t plo = (uint32_t)pidx, phi = (uint32_t)(pidx >> 32);
        uint32_t my_c = 0;
        for (int i = 0; i < cnt; ++i) {
            const int64_t p = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)phi, i) << 32) |
                                        (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)plo, i));
            float a0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), i));
            float a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), i));
            float a2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p2), i));
            // sources j-4 .. j-1 in path order; an absent source has weight 0: fl(e * 0) = +-0 leaves a value of [0, 255]
            // unchanged (a sum is -0 only when both terms are), and so does the clip after it
            const float w0 = rm_weight(p - q0), w1 = rm_weight(p - q1), w2 = rm_weight(p - q2), w3 = rm_weight(p - q3);
            a0 = rm_clamp255(__fadd_rn(a0, __fmul_rn(e0x, w0)));
            a1 = rm_clamp255(__fadd_rn(a1, __fmul_rn(e0y, w0)));
            a2 = rm_clamp255(__fadd_rn(a2, __fmul_rn(e0z, w0)));
            a0 = rm_clamp255(__fadd_rn(a0, __fmul_rn(e1x, w1)));
            a1 = rm_clamp255(__fadd_rn(a1, __fmul_rn(e1y, w1)));
            a2 = rm_clamp255(__fadd_rn(a2, __fmul_rn(e1z, w1)));
            a0 = rm_clamp255(__fadd_rn(a0, __fmul_rn(e2x, w2)));
            a1 = rm_clamp255(__fadd_rn(a1, __fmul_rn(e2y, w2)));
            a2 = rm_clamp255(__fadd_rn(a2, __fmul_rn(e2z, w2)));
            const float o0 = rm_clamp255(__fadd_rn(a0, __fmul_rn(e3x, w3)));  // the newest error: the dependency chain
            const float o1 = rm_clamp255(__fadd_rn(a1, __fmul_rn(e3y, w3)));
            const float o2 = rm_clamp255(__fadd_rn(a2, __fmul_rn(e3z, w3)));
            const float4 c = wave_nearest_record<CAP, M>(pal, pc, s_pal, wave_nearest<M>(pc, lane, o0, o1, o2), o0, o1, o2);
            if (lane == i) my_c = __float_as_uint(c.w);  // the lane that holds this step's position writes its colour
            q0 = q1;
            q1 = q2;
            q2 = q3;
            q3 = p;
            e0x = e1x;
            e0y = e1y;
            e0z = e1z;
            e1x = e2x;
            e1y = e2y;
            e1z = e2z;
            e2x = e3x;
            e2y = e3y;
            e2z = e3z;
            e3x = __fsub_rn(o0, c.x);
            e3y = __fsub_rn(o1, c.y);
            e3z = __fsub_rn(o2, c.z);
        }
        if (lane < cnt) {
            uint8_t *o = fout + ((size_t)row * uw + col) * 3;
            o[0] = (uint8_t)my_c;
            o[1] = (uint8_t)(my_c >> 8);
            o[2] = (uint8_t)(my_c >> 16);
        }
        cnt = ncnt;
        row = nrow;
        col = ncol;
        pidx = npidx;
        raw = nraw;
    }
}

}  // namespace

int launch_riemersma(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, const PalDev &pal, hipStream_t s)
{
    if (n_frames > 0x7fffffff) {
        set_error("dp_riemersma_u8: too many frames for one launch");
        return DP_EINVAL;
    }
    // dim = _next_power_of_two(max(h, w)) (dithering_lib.py:808-809): 1 for a 1 x 1 image
    const int64_t side = h > w ? h : w;
    int bits = 0;
    while (((int64_t)1 << bits) < side) ++bits;
    const size_t lds = pal.K > 64 ? (size_t)pal.K * 16 : 0;
    const bool big = pal.n_inner > kQueueSmall;
    ProfMark *pm = prof_begin(s);
#define DP_RM(C, MM)                                                                                                        \
    do {                                                                                                                    \
        auto kern = riemersma_kernel<C, MM>;                                                                                \
        DP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(kern, dim3((unsigned)n_frames), dim3(64), lds, s, in, out, h, w, bits, pal);                     \
    } while (0)
    if (pal.K <= 64) {
        if (big) DP_RM(kQueueLarge, 1); else DP_RM(kQueueSmall, 1);
    } else if (pal.K <= 256) {
        if (big) DP_RM(kQueueLarge, 4); else DP_RM(kQueueSmall, 4);
    } else {
        if (big) DP_RM(kQueueLarge, 16); else DP_RM(kQueueSmall, 16);
    }
#undef DP_RM
    prof_end(pm, s);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

}  // namespace dp
