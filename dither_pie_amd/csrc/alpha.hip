// Transparency (include/ditherpie_hip_alpha.h): the split of an RGBA source into RGB, mask and a count, the key index of an index
// plane, the join back to RGBA, and the descriptors of the two masked diffusions (their kernels are the MASKED instances of
// idiff_kernel and dotdiff_kernel: idiff.hip, dotdiff.hip).  The rules are stated by host_logic.h: alpha_split, alpha_key,
// alpha_join; the kernels here write the same bytes.
//
// alpha_split_kernel<VEC>, alpha_key_kernel<VEC>, alpha_join_kernel<VEC>   ONE launch per call, grid (ceil(h w / 1024), n_frames),
//   256 lanes; a lane owns a run of 4 consecutive pixels of one frame (in raster order: a run may cross the end of a row).  Pure
//   streaming: every byte is read once and written once.
//   VEC: every base is 4-byte aligned and h * w is a multiple of 4, so every run is complete and dword-aligned in every buffer
//   of every frame: 4 dwords of RGBA, 3 of RGB, 1 of mask or indices.  Otherwise (an odd address, a frame that cuts the last run)
//   the byte instance: the same registers, filled and stored byte by byte, nothing outside the frame touched.
//   masked[f]: a wave sums its transparent pixels (shuffles), the four sums meet in LDS and lane 0 adds them with one 64-bit atomic
//   per workgroup and frame (none when the sum is 0: the counters are cleared on the stream in front of the launch).
#include "dp_internal.h"

#include "../../include/ditherpie_hip_alpha.h"

namespace dp {
namespace {

constexpr int kAlphaThreads = 256;
constexpr int kAlphaRun = 4;   // pixels of a lane

// NDW dwords at p, of which the first nb bytes exist (VEC: all of them or none).  Bytes that are not loaded are 0.
template <bool VEC, int NDW>
__device__ __forceinline__ void alpha_load(const uint8_t *__restrict__ p, const int nb, uint32_t (&d)[NDW])
{
#pragma unroll
    for (int k = 0; k < NDW; ++k) d[k] = 0u;
    if (VEC) {
        if (nb) {
#pragma unroll
            for (int k = 0; k < NDW; ++k) d[k] = reinterpret_cast<const uint32_t *>(p)[k];
        }
    } else {
#pragma unroll
        for (int b = 0; b < 4 * NDW; ++b)
            if (b < nb) d[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
}

template <bool VEC, int NDW>
__device__ __forceinline__ void alpha_store(uint8_t *__restrict__ p, const int nb, const uint32_t (&d)[NDW])
{
    if (VEC) {
        if (nb) {
#pragma unroll
            for (int k = 0; k < NDW; ++k) reinterpret_cast<uint32_t *>(p)[k] = d[k];
        }
    } else {
#pragma unroll
        for (int b = 0; b < 4 * NDW; ++b)
            if (b < nb) p[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
    }
}

// the lane's run: its first pixel in the frame and how many of its pixels the frame has
struct AlphaRun { uint32_t i0; int nv; };
__device__ __forceinline__ AlphaRun alpha_run(const uint32_t px)
{
    const uint32_t i0 = ((uint32_t)blockIdx.x * kAlphaThreads + (uint32_t)threadIdx.x) * kAlphaRun;   // < 2^31 + 1024
    return {i0, i0 >= px ? 0 : (px - i0 < (uint32_t)kAlphaRun ? (int)(px - i0) : kAlphaRun)};
}

// four packed RGB pixels (24 bits each) as twelve bytes and back
__device__ __forceinline__ void pack_rgb(const uint32_t (&q)[4], uint32_t (&o)[3])
{
    o[0] = q[0] | (q[1] << 24);
    o[1] = (q[1] >> 8) | (q[2] << 16);
    o[2] = (q[2] >> 16) | (q[3] << 8);
}
__device__ __forceinline__ void unpack_rgb(const uint32_t (&o)[3], uint32_t (&q)[4])
{
    q[0] = o[0] & 0xFFFFFFu;
    q[1] = ((o[0] >> 24) | (o[1] << 8)) & 0xFFFFFFu;
    q[2] = ((o[1] >> 16) | (o[2] << 16)) & 0xFFFFFFu;
    q[3] = o[2] >> 8;
}

template <bool VEC>
__global__ __launch_bounds__(kAlphaThreads) void alpha_split_kernel(const uint8_t *__restrict__ rgba, const uint32_t px, const uint32_t w, const int bits,
                                                                     const uint32_t threshold, const uint32_t y0, const uint32_t x0, const int has_matte,
                                                                     const uint32_t matte, uint8_t *__restrict__ rgb, uint8_t *__restrict__ mask,
                                                                     unsigned long long *__restrict__ masked)
{
    __shared__ uint32_t s_sum[kAlphaThreads / 64];
    const AlphaRun run = alpha_run(px);
    const size_t at = (size_t)blockIdx.y * (size_t)px + (size_t)run.i0;   // the run's first pixel in the batch
    uint32_t count = 0;
    if (run.nv) {
        uint32_t src[4], q[4], o[3], mk[1] = {0u};
        alpha_load<VEC, 4>(rgba + at * 4u, 4 * run.nv, src);
        uint32_t y = bits ? run.i0 / w : 0u, x = bits ? run.i0 - y * w : 0u;
#pragma unroll
        for (int k = 0; k < kAlphaRun; ++k) {
            const uint32_t a = src[k] >> 24;
            uint32_t c = src[k] & 0xFFFFFFu;
            if (has_matte)
                c = alpha_matte(c & 255u, a, matte & 255u) | (alpha_matte((c >> 8) & 255u, a, (matte >> 8) & 255u) << 8) |
                    (alpha_matte(c >> 16, a, matte >> 16) << 16);
            q[k] = c;
            const uint32_t t = (k < run.nv && alpha_masked(bits, threshold, a, y0 + y, x0 + x)) ? 1u : 0u;
            mk[0] |= t << (8 * k);
            count += t;
            if (++x == w) x = 0u, ++y;
        }
        pack_rgb(q, o);
        alpha_store<VEC, 3>(rgb + at * 3u, 3 * run.nv, o);
        alpha_store<VEC, 1>(mask + at, run.nv, mk);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += (uint32_t)__shfl_xor((int)count, off);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (t) atomicAdd(&masked[blockIdx.y], (unsigned long long)t);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kAlphaThreads) void alpha_key_kernel(const uint8_t *planes, const uint8_t *__restrict__ mask, const uint32_t px,
                                                                   const uint32_t key, uint8_t *out)   // (out may be planes: no __restrict__)
{
    const AlphaRun run = alpha_run(px);
    if (!run.nv) return;
    const size_t at = (size_t)blockIdx.y * (size_t)px + (size_t)run.i0;
    uint32_t p[1], mk[1], o[1] = {0u};
    alpha_load<VEC, 1>(planes + at, run.nv, p);
    alpha_load<VEC, 1>(mask + at, run.nv, mk);
#pragma unroll
    for (int k = 0; k < kAlphaRun; ++k) o[0] |= (((mk[0] >> (8 * k)) & 255u) ? key : ((p[0] >> (8 * k)) & 255u)) << (8 * k);
    alpha_store<VEC, 1>(out + at, run.nv, o);
}

template <bool VEC>
__global__ __launch_bounds__(kAlphaThreads) void alpha_join_kernel(const uint8_t *__restrict__ rgb, const uint8_t *__restrict__ mask, const uint32_t px,
                                                                    const uint32_t fill, uint8_t *__restrict__ rgba)
{
    const AlphaRun run = alpha_run(px);
    if (!run.nv) return;
    const size_t at = (size_t)blockIdx.y * (size_t)px + (size_t)run.i0;
    uint32_t c[3], q[4], mk[1], o[4];
    alpha_load<VEC, 3>(rgb + at * 3u, 3 * run.nv, c);
    alpha_load<VEC, 1>(mask + at, run.nv, mk);
    unpack_rgb(c, q);
#pragma unroll
    for (int k = 0; k < kAlphaRun; ++k) o[k] = ((mk[0] >> (8 * k)) & 255u) ? fill : (q[k] | 0xFF000000u);
    alpha_store<VEC, 4>(rgba + at * 4u, 4 * run.nv, o);
}

bool overlap(const void *a, const size_t na, const void *b, const size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

dim3 alpha_grid(const int64_t n, const size_t px) { return dim3((unsigned)((px + kAlphaThreads * kAlphaRun - 1) / (kAlphaThreads * kAlphaRun)), (unsigned)n); }

bool alpha_vec(const size_t px, std::initializer_list<const void *> bases)
{
    uintptr_t all = (uintptr_t)px;
    for (const void *b : bases) all |= (uintptr_t)b;
    return (all & 3u) == 0;
}

const char *const kAlphaRule[] = {"", "n_frames must not be negative", "h and w must be >= 1 and h * w below 2^31", "at most 65535 frames per call",
                                  "mode must be 0 (threshold) or 1 (ordered)", "threshold must lie in 0 .. 256", "m must be one of 2, 4, 8",
                                  "y0 and x0 must lie in 0 .. 2^30"};

// struct_size and geometry of every descriptor -> DP_OK, or the refusal (its message names fn)
int check_alpha_head(const char *fn, const bool ok_size, const size_t want, const int64_t n, const int h, const int w)
{
    if (!ok_size) {
        set_error("%s: bad argument (a NULL descriptor or a struct_size that is not %zu)", fn, want);
        return DP_EINVAL;
    }
    if (const int bad = alpha_geometry_rule(n, h, w)) {
        set_error("%s: %s (n_frames %lld, %d x %d)", fn, kAlphaRule[bad], (long long)n, h, w);
        return bad == 3 ? DP_EUNSUPPORTED : DP_EINVAL;
    }
    return DP_OK;
}

struct AlphaBuf { const void *p; size_t bytes; };

// no output overlaps an input or another output (same_ok: the one pair that may be the same buffer)
int check_alpha_overlap(const char *fn, std::initializer_list<AlphaBuf> in, std::initializer_list<AlphaBuf> out, const void *same_ok = nullptr)
{
    for (auto o = out.begin(); o != out.end(); ++o) {
        for (const AlphaBuf &i : in)
            if (overlap(o->p, o->bytes, i.p, i.bytes) && !(same_ok && o->p == same_ok && i.p == same_ok)) {
                set_error("%s: bad argument (an output overlaps an input)", fn);
                return DP_EINVAL;
            }
        for (auto q = o + 1; q != out.end(); ++q)
            if (overlap(o->p, o->bytes, q->p, q->bytes)) {
                set_error("%s: bad argument (the outputs overlap each other)", fn);
                return DP_EINVAL;
            }
    }
    return DP_OK;
}

int check_split(const char *fn, const dp_alpha_split_args *a)
{
    if (const int rc = check_alpha_head(fn, a && a->struct_size == sizeof(*a), sizeof(*a), a ? a->n_frames : 0, a ? a->h : 1, a ? a->w : 1)) return rc;
    if (const int bad = alpha_split_rule(a->mode, a->threshold, a->m, a->y0, a->x0)) {
        set_error("%s: %s (mode %d, threshold %d, m %d, origin %d, %d)", fn, kAlphaRule[bad], a->mode, a->threshold, a->m, a->y0, a->x0);
        return DP_EINVAL;
    }
    if (a->n_frames == 0) return DP_OK;
    if (!a->rgba_dev || !a->rgb_dev || !a->mask_dev || !a->masked_dev) {
        set_error("%s: bad argument (a NULL buffer)", fn);
        return DP_EINVAL;
    }
    if ((uintptr_t)a->masked_dev & 7u) {
        set_error("%s: masked_dev must be 8-byte aligned", fn);
        return DP_EINVAL;
    }
    const size_t t = (size_t)a->n_frames * (size_t)a->h * (size_t)a->w;
    return check_alpha_overlap(fn, {{a->rgba_dev, 4u * t}}, {{a->rgb_dev, 3u * t}, {a->mask_dev, t}, {a->masked_dev, 8u * (size_t)a->n_frames}});
}

int check_key(const char *fn, const dp_alpha_key_args *a)
{
    if (const int rc = check_alpha_head(fn, a && a->struct_size == sizeof(*a), sizeof(*a), a ? a->n_frames : 0, a ? a->h : 1, a ? a->w : 1)) return rc;
    if (a->key < 0 || a->key > 255) {
        set_error("%s: key must lie in 0 .. 255, not %d", fn, a->key);
        return DP_EINVAL;
    }
    if (a->n_frames == 0) return DP_OK;
    if (!a->planes_dev || !a->mask_dev || !a->out_dev) {
        set_error("%s: bad argument (a NULL buffer)", fn);
        return DP_EINVAL;
    }
    const size_t t = (size_t)a->n_frames * (size_t)a->h * (size_t)a->w;
    return check_alpha_overlap(fn, {{a->planes_dev, t}, {a->mask_dev, t}}, {{a->out_dev, t}}, a->planes_dev);
}

int check_join(const char *fn, const dp_alpha_join_args *a)
{
    if (const int rc = check_alpha_head(fn, a && a->struct_size == sizeof(*a), sizeof(*a), a ? a->n_frames : 0, a ? a->h : 1, a ? a->w : 1)) return rc;
    if (a->n_frames == 0) return DP_OK;
    if (!a->rgb_dev || !a->mask_dev || !a->rgba_dev) {
        set_error("%s: bad argument (a NULL buffer)", fn);
        return DP_EINVAL;
    }
    const size_t t = (size_t)a->n_frames * (size_t)a->h * (size_t)a->w;
    return check_alpha_overlap(fn, {{a->rgb_dev, 3u * t}, {a->mask_dev, t}}, {{a->rgba_dev, 4u * t}});
}

uint32_t pack3(const uint8_t *c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_alpha_split_u8(const dp_alpha_split_args *a)
{
    if (const int rc = check_split("dp_alpha_split_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    hipStream_t s = (hipStream_t)a->stream;
    const size_t px = (size_t)a->h * (size_t)a->w;
    ProfMark *pm = prof_begin(s);
    DP_HIP(hipMemsetAsync(a->masked_dev, 0, (size_t)a->n_frames * sizeof(int64_t), s));
    unsigned long long *masked = reinterpret_cast<unsigned long long *>(a->masked_dev);
    const int bits = alpha_bits(a->mode, a->m);
    const uint32_t thr = a->mode == DP_ALPHA_THRESHOLD ? (uint32_t)a->threshold : 0u, y0 = bits ? (uint32_t)a->y0 : 0u, x0 = bits ? (uint32_t)a->x0 : 0u;
    if (alpha_vec(px, {a->rgba_dev, a->rgb_dev, a->mask_dev}))
        hipLaunchKernelGGL((alpha_split_kernel<true>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->rgba_dev, (uint32_t)px, (uint32_t)a->w, bits, thr,
                           y0, x0, a->has_matte ? 1 : 0, pack3(a->matte), a->rgb_dev, a->mask_dev, masked);
    else
        hipLaunchKernelGGL((alpha_split_kernel<false>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->rgba_dev, (uint32_t)px, (uint32_t)a->w, bits, thr,
                           y0, x0, a->has_matte ? 1 : 0, pack3(a->matte), a->rgb_dev, a->mask_dev, masked);
    DP_HIP(hipGetLastError());
    prof_end(pm, s);
    return DP_OK;
}

int dp_alpha_split_host_u8(const dp_alpha_split_args *a)
{
    if (const int rc = check_split("dp_alpha_split_host_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    alpha_split(a->rgba_dev, a->n_frames, a->h, a->w, a->mode, a->threshold, a->m, a->mode == DP_ALPHA_ORDERED ? a->y0 : 0,
                a->mode == DP_ALPHA_ORDERED ? a->x0 : 0, a->has_matte != 0, a->matte, a->rgb_dev, a->mask_dev, a->masked_dev);
    return DP_OK;
}

int dp_alpha_key_u8(const dp_alpha_key_args *a)
{
    if (const int rc = check_key("dp_alpha_key_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    hipStream_t s = (hipStream_t)a->stream;
    const size_t px = (size_t)a->h * (size_t)a->w;
    ProfMark *pm = prof_begin(s);
    if (alpha_vec(px, {a->planes_dev, a->mask_dev, a->out_dev}))
        hipLaunchKernelGGL((alpha_key_kernel<true>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->planes_dev, a->mask_dev, (uint32_t)px,
                           (uint32_t)a->key, a->out_dev);
    else
        hipLaunchKernelGGL((alpha_key_kernel<false>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->planes_dev, a->mask_dev, (uint32_t)px,
                           (uint32_t)a->key, a->out_dev);
    DP_HIP(hipGetLastError());
    prof_end(pm, s);
    return DP_OK;
}

int dp_alpha_key_host_u8(const dp_alpha_key_args *a)
{
    if (const int rc = check_key("dp_alpha_key_host_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    alpha_key(a->planes_dev, a->mask_dev, (size_t)a->n_frames * (size_t)a->h * (size_t)a->w, a->key, a->out_dev);
    return DP_OK;
}

int dp_alpha_join_u8(const dp_alpha_join_args *a)
{
    if (const int rc = check_join("dp_alpha_join_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    hipStream_t s = (hipStream_t)a->stream;
    const size_t px = (size_t)a->h * (size_t)a->w;
    ProfMark *pm = prof_begin(s);
    if (alpha_vec(px, {a->rgb_dev, a->mask_dev, a->rgba_dev}))
        hipLaunchKernelGGL((alpha_join_kernel<true>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->rgb_dev, a->mask_dev, (uint32_t)px, pack3(a->fill),
                           a->rgba_dev);
    else
        hipLaunchKernelGGL((alpha_join_kernel<false>), alpha_grid(a->n_frames, px), dim3(kAlphaThreads), 0, s, a->rgb_dev, a->mask_dev, (uint32_t)px, pack3(a->fill),
                           a->rgba_dev);
    DP_HIP(hipGetLastError());
    prof_end(pm, s);
    return DP_OK;
}

int dp_alpha_join_host_u8(const dp_alpha_join_args *a)
{
    if (const int rc = check_join("dp_alpha_join_host_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    alpha_join(a->rgb_dev, a->mask_dev, (size_t)a->n_frames * (size_t)a->h * (size_t)a->w, a->fill, a->rgba_dev);
    return DP_OK;
}

// The masked diffusions: the descriptor is unpacked here, the checks and the launch are those of dp_idiff_u8 / dp_dotdiff_u8
// (idiff.hip: idiff_call, dotdiff.hip: dotdiff_call), which name this function in their refusals.
int dp_alpha_idiff_u8(const dp_alpha_idiff_args *a)
{
    static const char fn[] = "dp_alpha_idiff_u8";
    if (!a || a->struct_size != sizeof(*a)) {
        set_error("%s: bad argument (a NULL descriptor or a struct_size that is not %zu)", fn, sizeof(*a));
        return DP_EINVAL;
    }
    return idiff_call(fn, true, a->in_dev, a->mask_dev, pack3(a->fill), a->out_dev, a->n_frames, a->h, a->w, a->pal, a->dx, a->dy, a->weight, a->n_taps,
                      a->divisor, a->strength256, a->workspace_dev, a->workspace_bytes, a->stream);
}

int dp_alpha_dotdiff_u8(const dp_alpha_dotdiff_args *a)
{
    static const char fn[] = "dp_alpha_dotdiff_u8";
    if (!a || a->struct_size != sizeof(*a)) {
        set_error("%s: bad argument (a NULL descriptor or a struct_size that is not %zu)", fn, sizeof(*a));
        return DP_EINVAL;
    }
    return dotdiff_call(fn, true, a->in_dev, a->mask_dev, pack3(a->fill), a->out_dev, a->n_frames, a->h, a->w, a->pal, a->classes_host, a->m, a->strength256,
                        a->stream);
}

}  // extern "C"
