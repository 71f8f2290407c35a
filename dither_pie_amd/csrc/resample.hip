// Filtered resize (include/ditherpie_hip_resample.h): Pillow's BOX / BILINEAR / HAMMING / BICUBIC / LANCZOS resize of packed RGB
// uint8 frames, bit for bit.  The coefficients are built on the host (host_logic.h: resample_plan) and live on the device as two
// tables per axis: bounds[out] = (first source position, count) and kk[out][ksize] int32 in 1 / 2^22.  A resize is one or two
// launches: the horizontal pass over the source rows the vertical pass reads, into a uint8 intermediate (the workspace), then the
// vertical pass.  Every kernel computes clamp((2^21 + sum src * k) >> 22, 0, 255) in int32; a plan's sums fit (the planner refuses
// the others).  Frames may sit at any byte address: the dword accesses below are unaligned ones that stay inside a row.
//
// resample_v_kernel        a lane owns four consecutive bytes of an output row (ow * 3 flat bytes: channels do not matter to a
//   vertical pass).  blockIdx.y is the output row, so its first source row, its count and its coefficients are wave-uniform:
//   scalar loads, the coefficient a scalar operand of the multiply-adds.  Per tap one coalesced dword load of the source row; the
//   last 1 .. 3 bytes of a row go bytewise.
// resample_h_naive_kernel  a lane per output pixel, byte reads from global memory.  Serves every plan; the planner gives it BOX,
//   BILINEAR and HAMMING (nothing or little to reuse) and windows wider than a staged row (LANCZOS 400 -> 2).
// resample_h_staged_kernel one wave per block of kResampleStageRows source rows x kResampleStageCols output columns.  The source
//   span of those columns is copied to LDS with coalesced dword loads at an odd dword pitch; then a lane owns a ROW of the block
//   and the wave walks the output columns, so the window and its coefficients are wave-uniform and the 64 byte reads of a tap hit
//   64 different banks.  The results go through LDS once more and leave as coalesced dwords.
// The products: v_mad_i32_i24 (a byte times |k| < 2^23), or the instance with 32-bit multiplies for a plan with max |k| >= 2^23.
#include "dp_internal.h"

#include <algorithm>
#include <cstring>

#include "../../include/ditherpie_hip_resample.h"

struct dp_resample_plan {
    dp::ResamplePlanHost host;   // (the coefficient vectors are dropped after the upload; the bounds stay)
    void *blob;                  // the one allocation behind the four tables
    const int2 *vb, *hb;         // bounds of the vertical / horizontal pass
    const int32_t *vk, *hk;      // their coefficients
    int h_pitch;                 // staged horizontal kernel: dwords per LDS row (odd), 0 = its spans do not fit: naive only
    int device;
};

namespace dp {
namespace {

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
constexpr int kHalf = 1 << (kResampleBits - 1);

template <bool MUL32>
__device__ __forceinline__ int mac(const int s, const uint32_t v, const int k)
{
    if (MUL32) return s + (int)v * k;
    return __mul24((int)v, k) + s;   // v_mad_i32_i24
}

// clamp(s >> 22, 0, 255), clamped BEFORE the shift: written as shift-then-clamp, two neighbouring bytes of the vertical kernel's
// dword are fused by hipcc into gfx950's v_ashr_pk_u8_i32, whose result it then ORs with the other two bytes as if bits 16 .. 31
// were zero; on the device they are not (bytes 2 and 3 of every dword came out wrong, bytes 0 and 1 right)
__device__ __forceinline__ uint32_t clamp8(const int s) { return (uint32_t)min(max(s, 0), (256 << kResampleBits) - 1) >> kResampleBits; }

template <bool MUL32>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const size_t in_frame,
                                                         const size_t out_frame, const int rb, const int2 *__restrict__ bounds,
                                                         const int32_t *__restrict__ kk, const int ksize, const int yoff)
{
    const int oy = blockIdx.y;
    const int2 b = bounds[oy];
    const int32_t *__restrict__ k = kk + (size_t)oy * (size_t)ksize;
    const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= rb) return;
    const uint8_t *src = in + (size_t)blockIdx.z * in_frame + (size_t)(b.x - yoff) * (size_t)rb + (size_t)j;
    uint8_t *dst = out + (size_t)blockIdx.z * out_frame + (size_t)oy * (size_t)rb + (size_t)j;
    int s0 = kHalf, s1 = kHalf, s2 = kHalf, s3 = kHalf;
    if (j + 4 <= rb) {
#pragma unroll 4
        for (int y = 0; y < b.y; ++y) {
            const uint32_t v = *reinterpret_cast<const u32_unaligned *>(src + (size_t)y * (size_t)rb);
            const int c = k[y];
            s0 = mac<MUL32>(s0, v & 255u, c);
            s1 = mac<MUL32>(s1, (v >> 8) & 255u, c);
            s2 = mac<MUL32>(s2, (v >> 16) & 255u, c);
            s3 = mac<MUL32>(s3, v >> 24, c);
        }
        *reinterpret_cast<u32_unaligned *>(dst) = clamp8(s0) | (clamp8(s1) << 8) | (clamp8(s2) << 16) | (clamp8(s3) << 24);
    } else {   // the last 1 .. 3 bytes of the row
        const int nb = rb - j;
        for (int y = 0; y < b.y; ++y) {
            const uint8_t *p = src + (size_t)y * (size_t)rb;
            const int c = k[y];
            s0 = mac<MUL32>(s0, p[0], c);
            if (nb > 1) s1 = mac<MUL32>(s1, p[1], c);
            if (nb > 2) s2 = mac<MUL32>(s2, p[2], c);
        }
        dst[0] = (uint8_t)clamp8(s0);
        if (nb > 1) dst[1] = (uint8_t)clamp8(s1);
        if (nb > 2) dst[2] = (uint8_t)clamp8(s2);
    }
}

// in points at the first source row of the pass (row y0 of a frame), out at row 0 of the intermediate / the output
template <bool MUL32>
__global__ __launch_bounds__(256) void resample_h_naive_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const size_t in_frame,
                                                               const size_t out_frame, const int w, const int ow,
                                                               const int2 *__restrict__ bounds, const int32_t *__restrict__ kk, const int ksize)
{
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= ow) return;
    const int r = blockIdx.y;
    const int2 b = bounds[ox];
    const int32_t *__restrict__ k = kk + (size_t)ox * (size_t)ksize;
    const uint8_t *src = in + (size_t)blockIdx.z * in_frame + ((size_t)r * (size_t)w + (size_t)b.x) * 3u;
    int s0 = kHalf, s1 = kHalf, s2 = kHalf;
    for (int x = 0; x < b.y; ++x) {
        const int c = k[x];
        s0 = mac<MUL32>(s0, src[3 * x], c);
        s1 = mac<MUL32>(s1, src[3 * x + 1], c);
        s2 = mac<MUL32>(s2, src[3 * x + 2], c);
    }
    uint8_t *dst = out + (size_t)blockIdx.z * out_frame + ((size_t)r * (size_t)ow + (size_t)ox) * 3u;
    dst[0] = (uint8_t)clamp8(s0);
    dst[1] = (uint8_t)clamp8(s1);
    dst[2] = (uint8_t)clamp8(s2);
}

constexpr int kOutPitch = kResampleStageCols * 3 / 4 + 1;   // dwords per row of the staged results: 12 used, 13 is odd

template <bool MUL32>
__global__ __launch_bounds__(64) void resample_h_staged_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const size_t in_frame,
                                                               const size_t out_frame, const int w, const int rows, const int ow,
                                                               const int2 *__restrict__ bounds, const int32_t *__restrict__ kk, const int ksize,
                                                               const int pitch)
{
    extern __shared__ uint32_t s_src[];   // [kResampleStageRows][pitch]
    __shared__ uint32_t s_res[kResampleStageRows * kOutPitch];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * kResampleStageCols, c1 = min(ow, c0 + kResampleStageCols);
    const int r0 = blockIdx.y * kResampleStageRows, nr = min(kResampleStageRows, rows - r0);
    // first source positions and ends are non-decreasing in the output position: the span of the block
    const int2 bl = bounds[c0], bh = bounds[c1 - 1];
    const int lo = bl.x, nbytes = (bh.x + bh.y - lo) * 3;   // <= 4 * pitch (host_logic.h: resample_h_pitch)
    const int ndw = (nbytes + 3) >> 2;
    const uint8_t *src = in + (size_t)blockIdx.z * in_frame + ((size_t)r0 * (size_t)w + (size_t)lo) * 3u;
    for (int i = lane; i < nr * ndw; i += 64) {
        const int rr = i / ndw, d = i - rr * ndw;
        const uint8_t *p = src + (size_t)rr * (size_t)w * 3u + (size_t)d * 4u;
        uint32_t v;
        if (4 * d + 4 <= nbytes) {
            v = *reinterpret_cast<const u32_unaligned *>(p);
        } else {   // the last dword of a row's span stops at the span's bytes
            v = 0;
            for (int bb = 0; bb < nbytes - 4 * d; ++bb) v |= (uint32_t)p[bb] << (8 * bb);
        }
        s_src[rr * pitch + d] = v;
    }
    __syncthreads();
    if (lane < nr) {
        const uint8_t *row = reinterpret_cast<const uint8_t *>(s_src + lane * pitch);
        uint8_t *res = reinterpret_cast<uint8_t *>(s_res + lane * kOutPitch);
        for (int c = c0; c < c1; ++c) {
            const int2 b = bounds[c];
            const int32_t *__restrict__ k = kk + (size_t)c * (size_t)ksize;
            const uint8_t *p = row + (b.x - lo) * 3;
            int s0 = kHalf, s1 = kHalf, s2 = kHalf;
            for (int x = 0; x < b.y; ++x) {
                const int cf = k[x];
                s0 = mac<MUL32>(s0, p[3 * x], cf);
                s1 = mac<MUL32>(s1, p[3 * x + 1], cf);
                s2 = mac<MUL32>(s2, p[3 * x + 2], cf);
            }
            res[3 * (c - c0)] = (uint8_t)clamp8(s0);
            res[3 * (c - c0) + 1] = (uint8_t)clamp8(s1);
            res[3 * (c - c0) + 2] = (uint8_t)clamp8(s2);
        }
    }
    __syncthreads();
    uint8_t *dst = out + (size_t)blockIdx.z * out_frame + ((size_t)r0 * (size_t)ow + (size_t)c0) * 3u;
    const int ob = (c1 - c0) * 3;
    if (ob == kResampleStageCols * 3) {
        constexpr int DW = kResampleStageCols * 3 / 4;
        for (int i = lane; i < nr * DW; i += 64) {
            const int rr = i / DW, d = i - rr * DW;
            *reinterpret_cast<u32_unaligned *>(dst + (size_t)rr * (size_t)ow * 3u + (size_t)d * 4u) = s_res[rr * kOutPitch + d];
        }
    } else {   // the last, narrower group of columns
        for (int i = lane; i < nr * ob; i += 64) {
            const int rr = i / ob, bb = i - rr * ob;
            dst[(size_t)rr * (size_t)ow * 3u + (size_t)bb] = reinterpret_cast<const uint8_t *>(s_res + rr * kOutPitch)[bb];
        }
    }
}

// dwords per LDS row the staged kernel needs for this plan (odd), or 0: a span does not fit kResampleStagePitch
int resample_h_pitch(const ResampleAxis &hor)
{
    if (!resample_h_fits(hor)) return 0;
    int need = 1;
    for (int c0 = 0; c0 < hor.out; c0 += kResampleStageCols) {
        const int c1 = std::min(hor.out, c0 + kResampleStageCols);
        const int span = hor.bounds[2 * (size_t)(c1 - 1)] + hor.bounds[2 * (size_t)(c1 - 1) + 1] - hor.bounds[2 * (size_t)c0];
        need = std::max(need, (span * 3 + 3) / 4);
    }
    return std::min(need | 1, kResampleStagePitch);
}

template <bool MUL32>
int launch_passes(const dp_resample_plan *pl, const uint8_t *in, uint8_t *out, const int64_t n, uint8_t *mid, const bool staged, hipStream_t s)
{
    const ResamplePlanHost &p = pl->host;
    const size_t fin = 3 * (size_t)p.h * (size_t)p.w, fout = 3 * (size_t)p.oh * (size_t)p.ow;
    const int rows = p.need_v ? p.y1 - p.y0 : p.h;   // rows of the horizontal pass
    const size_t fmid = 3 * (size_t)rows * (size_t)p.ow;
    for (int64_t f0 = 0; f0 < n; f0 += 65535) {
        const unsigned nf = (unsigned)std::min<int64_t>(65535, n - f0);
        const uint8_t *src = in + (size_t)f0 * fin;
        uint8_t *dst = out + (size_t)f0 * fout;
        ProfMark *pm = prof_begin(s);
        const uint8_t *vsrc = src;
        size_t vframe = fin;
        int yoff = 0;
        if (p.need_h) {
            uint8_t *hdst = p.need_v ? mid + (size_t)f0 * fmid : dst;
            const uint8_t *hsrc = src + 3 * (size_t)(p.need_v ? p.y0 : 0) * (size_t)p.w;
            if (staged)
                hipLaunchKernelGGL((resample_h_staged_kernel<MUL32>), dim3((p.ow + kResampleStageCols - 1) / kResampleStageCols,
                                   (rows + kResampleStageRows - 1) / kResampleStageRows, nf), dim3(64), sizeof(uint32_t) * kResampleStageRows * (size_t)pl->h_pitch,
                                   s, hsrc, hdst, fin, p.need_v ? fmid : fout, p.w, rows, p.ow, pl->hb, pl->hk, p.hor.ksize, pl->h_pitch);
            else
                hipLaunchKernelGGL((resample_h_naive_kernel<MUL32>), dim3((p.ow + 255) / 256, rows, nf), dim3(256), 0, s, hsrc, hdst, fin,
                                   p.need_v ? fmid : fout, p.w, p.ow, pl->hb, pl->hk, p.hor.ksize);
            DP_HIP(hipGetLastError());
            vsrc = hdst;
            vframe = fmid;
            yoff = p.y0;
        }
        prof_mid(pm, s);
        if (p.need_v) {
            const int rb = 3 * p.ow;   // (ow == w when there was no horizontal pass)
            hipLaunchKernelGGL((resample_v_kernel<MUL32>), dim3(((rb + 3) / 4 + 255) / 256, p.oh, nf), dim3(256), 0, s, vsrc, dst, vframe, fout, rb, pl->vb,
                               pl->vk, p.ver.ksize, yoff);
            DP_HIP(hipGetLastError());
        }
        prof_end(pm, s);
    }
    return DP_OK;
}

size_t resample_ws_bytes(const dp_resample_plan *pl, const int64_t n)
{
    if (!pl || n < 1 || !(pl->host.need_h && pl->host.need_v)) return 0;
    const size_t b = (size_t)n * 3u * (size_t)(pl->host.y1 - pl->host.y0) * (size_t)pl->host.ow;
    return (b + 15u) & ~(size_t)15u;
}

const char *const kPlanRule[] = {"", "the filter must be one of box, bilinear, hamming, bicubic, lanczos (0 .. 4)",
                                 "every size must lie in 1 .. 16384 and h * w must not exceed 2^30",
                                 "the 32-bit sum of a pass could overflow with these coefficients"};

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_resample_plan_create(int filter, int h, int w, int oh, int ow, dp_resample_plan **out)
{
    if (!out) {
        set_error("dp_resample_plan_create: bad argument (out is NULL)");
        return DP_EINVAL;
    }
    *out = nullptr;
    dp_resample_plan *pl = new dp_resample_plan();
    if (const int bad = resample_plan(filter, h, w, oh, ow, pl->host)) {
        set_error("dp_resample_plan_create: %s (filter %d, %d x %d -> %d x %d)", kPlanRule[bad], filter, h, w, oh, ow);
        delete pl;
        return bad == 3 ? DP_EUNSUPPORTED : DP_EINVAL;
    }
    ResamplePlanHost &p = pl->host;
    pl->h_pitch = p.need_h ? resample_h_pitch(p.hor) : 0;
    // one blob: vertical bounds, horizontal bounds, vertical k, horizontal k (all 4-byte items; the bounds are int2, 8-byte aligned)
    const size_t nvb = p.ver.bounds.size(), nhb = p.hor.bounds.size(), nvk = p.ver.kk.size(), nhk = p.hor.kk.size();
    std::vector<int32_t> blob;
    blob.reserve(nvb + nhb + nvk + nhk);
    blob.insert(blob.end(), p.ver.bounds.begin(), p.ver.bounds.end());
    blob.insert(blob.end(), p.hor.bounds.begin(), p.hor.bounds.end());
    blob.insert(blob.end(), p.ver.kk.begin(), p.ver.kk.end());
    blob.insert(blob.end(), p.hor.kk.begin(), p.hor.kk.end());
    hipError_t e = hipGetDevice(&pl->device);
    if (e == hipSuccess) e = hipMalloc(&pl->blob, sizeof(int32_t) * blob.size());
    if (e == hipSuccess) e = hipMemcpy(pl->blob, blob.data(), sizeof(int32_t) * blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (pl->blob) (void)hipFree(pl->blob);
        delete pl;
        return hip_fail(e, "dp_resample_plan_create upload");
    }
    const int32_t *base = static_cast<const int32_t *>(pl->blob);
    pl->vb = reinterpret_cast<const int2 *>(base);
    pl->hb = reinterpret_cast<const int2 *>(base + nvb);
    pl->vk = base + nvb + nhb;
    pl->hk = base + nvb + nhb + nvk;
    std::vector<int32_t>().swap(p.ver.kk);
    std::vector<int32_t>().swap(p.hor.kk);
    *out = pl;
    return DP_OK;
}

void dp_resample_plan_destroy(dp_resample_plan *plan)
{
    if (!plan) return;
    if (plan->blob) (void)hipFree(plan->blob);
    delete plan;
}

size_t dp_resample_workspace_bytes(const dp_resample_plan *plan, int64_t n_frames) { return resample_ws_bytes(plan, n_frames); }

int dp_resample_u8(const dp_resample_args *a)
{
    if (!a || a->struct_size != sizeof(dp_resample_args)) {
        set_error("dp_resample_u8: bad argument (a NULL descriptor or a struct_size that is not %zu)", sizeof(dp_resample_args));
        return DP_EINVAL;
    }
    const size_t need = a->plan && a->n_frames > 0 ? resample_ws_bytes(a->plan, a->n_frames) : 0;
    if (!a->plan || a->n_frames < 0 || (a->n_frames > 0 && (!a->in_dev || !a->out_dev || (need && !a->workspace_dev)))) {
        set_error("dp_resample_u8: bad argument (pointers, n_frames >= 0)");
        return DP_EINVAL;
    }
    if (a->in_dev && a->out_dev == a->in_dev) {
        set_error("dp_resample_u8: out_dev must not be in_dev");
        return DP_EINVAL;
    }
    if (a->workspace_dev && ((uintptr_t)a->workspace_dev & 15u)) {
        set_error("dp_resample_u8: the workspace must be 16-byte aligned");
        return DP_EINVAL;
    }
    if (a->n_frames == 0) return DP_OK;
    if (a->workspace_bytes < need) {
        set_error("dp_resample_u8: workspace too small (need %zu bytes)", need);
        return DP_EWORKSPACE;
    }
    const dp_resample_plan *pl = a->plan;
    const ResamplePlanHost &p = pl->host;
    hipStream_t s = (hipStream_t)a->stream;
    if (!p.need_h && !p.need_v) {   // equal sizes on both axes: a copy
        DP_HIP(hipMemcpyAsync(a->out_dev, a->in_dev, (size_t)a->n_frames * 3u * (size_t)p.h * (size_t)p.w, hipMemcpyDeviceToDevice, s));
        return DP_OK;
    }
    bool mul32 = p.mul32, staged = p.h_kernel == kResampleHStaged && pl->h_pitch > 0;
    // experiments build: DP_RESAMPLE_MUL32=1 takes the 32-bit-multiply instance for any plan; DP_RESAMPLE_H=naive / staged takes
    // that horizontal kernel whatever the planner's rule says (staged: where the spans fit a staged row; the A/B of
    // tools/bench_scripts/resample_bench.py)
    if (const char *e = exp_env("DP_RESAMPLE_MUL32")) mul32 = mul32 || std::atoi(e) != 0;
    if (const char *e = exp_env("DP_RESAMPLE_H")) staged = std::strcmp(e, "naive") != 0 && (std::strcmp(e, "staged") == 0 || staged) && pl->h_pitch > 0;
    uint8_t *mid = static_cast<uint8_t *>(a->workspace_dev);
    return mul32 ? launch_passes<true>(pl, a->in_dev, a->out_dev, a->n_frames, mid, staged, s)
                 : launch_passes<false>(pl, a->in_dev, a->out_dev, a->n_frames, mid, staged, s);
}

int dp_resample_host(int filter, const uint8_t *in, uint8_t *out, int64_t n, int h, int w, int oh, int ow)
{
    if (n < 0 || (n > 0 && (!in || !out))) {
        set_error("dp_resample_host: bad argument (pointers, n >= 0)");
        return DP_EINVAL;
    }
    ResamplePlanHost p;
    if (const int bad = resample_plan(filter, h, w, oh, ow, p)) {
        set_error("dp_resample_host: %s (filter %d, %d x %d -> %d x %d)", kPlanRule[bad], filter, h, w, oh, ow);
        return bad == 3 ? DP_EUNSUPPORTED : DP_EINVAL;
    }
    resample_host(p, in, out, n);
    return DP_OK;
}

}  // extern "C"
