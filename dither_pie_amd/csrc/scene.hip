// Scene-cut detection (include/ditherpie_hip_scene.h): a coarse colour signature per frame and the L1 distance between the
// signatures of consecutive frames.
//
// frame_signature_kernel   grid (blocks per frame, frames): every workgroup counts its share of one frame's pixels into a
//                          4096 x uint32 histogram in LDS (16 KB, LDS atomics) over the 16^3 cells of the colour cube -- the
//                          cell id of kmeans_hist.hip -- and then adds its non-zero bins to the frame's row of the signature
//                          buffer with global atomics.  Pixels are loaded as index_from_rgb_kernel (indexed.hip) loads them:
//                          four per lane as one 12-byte load where the frame's base is 4-byte aligned, one per lane otherwise
//                          and for the last n_px % 4.  On coherent content the lanes of a wave mostly hit ONE bin: while at
//                          least eight whole-group lanes agree with the first pending one, one lane adds for all of them (as
//                          hist_count_kernel does), so a flat frame costs one LDS atomic per wave and group, not 64 on one
//                          address.  Integer adds: the result does not depend on the order.
// signature_distance_kernel  one workgroup per pair of signatures: 16 bins per lane (four uint4), |a - b| summed in 64 bits,
//                          a wave reduction, then the four wave sums through LDS.
#include "dp_internal.h"

#include "../../include/ditherpie_hip_scene.h"

namespace dp {
namespace {

constexpr int kBins = 4096;
constexpr int kSigThreads = 256;
constexpr int kSigGroupsPerLane = 16;    // 12-byte groups a lane gets before a frame is given another workgroup ...
constexpr int kSigMaxBlocksPerFrame = 64;   // ... up to this many (a flush is up to 4096 global atomics per workgroup)
constexpr int kDistThreads = 256;

struct alignas(4) Word3 {
    uint32_t x, y, z;
};

__device__ __forceinline__ uint32_t cell_of(const uint32_t v)   // v = r | g << 8 | b << 16  ->  r' << 8 | g' << 4 | b'
{
    return ((v & 0xf0u) << 4) | ((v & 0xf000u) >> 8) | ((v & 0xf00000u) >> 20);
}

__global__ __launch_bounds__(kSigThreads) void frame_signature_kernel(const uint8_t *__restrict__ frames, const long long n_px,
                                                                      uint32_t *__restrict__ sig)
{
    __shared__ uint32_t s_cnt[kBins];
    for (int i = threadIdx.x; i < kBins; i += kSigThreads) s_cnt[i] = 0u;
    __syncthreads();
    const uint8_t *__restrict__ rgb = frames + (size_t)blockIdx.y * 3u * (size_t)n_px;
    const long long gid = (long long)blockIdx.x * kSigThreads + threadIdx.x, stride = (long long)gridDim.x * kSigThreads;
    const int lane = (int)(threadIdx.x & 63u);
    long long scalar_from = 0;
    if (((uintptr_t)rgb & 3u) == 0) {   // (uniform over the workgroup: a property of the frame's base)
        const long long n4 = n_px >> 2;
        for (long long g = gid; g < n4; g += stride) {
            const Word3 p = reinterpret_cast<const Word3 *>(rgb)[g];
            const uint32_t c0 = cell_of(p.x), c1 = cell_of((p.x >> 24) | (p.y << 8)), c2 = cell_of((p.y >> 16) | (p.z << 16)),
                           c3 = cell_of(p.z >> 8);
            const bool all4 = c0 == c1 && c1 == c2 && c2 == c3;
            bool done = false;
            unsigned long long pend = __ballot(all4);
            for (int round = 0; round < 3 && __popcll(pend) >= 8; ++round) {   // (wave-uniform)
                const int leader = __ffsll((long long)pend) - 1;
                const uint32_t lc = (uint32_t)__builtin_amdgcn_readlane((int)c0, leader);
                const unsigned long long m = __ballot(all4 && !done && c0 == lc);
                if (lane == leader) atomicAdd(&s_cnt[lc], 4u * (uint32_t)__popcll(m));
                if ((m >> lane) & 1ull) done = true;
                pend &= ~m;
            }
            if (done) continue;
            // a lane's run of one cell costs one LDS atomic
            if (all4) {
                atomicAdd(&s_cnt[c0], 4u);
            } else {
                uint32_t run = 1;
                if (c1 == c0) ++run;
                else { atomicAdd(&s_cnt[c0], run); run = 1; }
                if (c2 == c1) ++run;
                else { atomicAdd(&s_cnt[c1], run); run = 1; }
                if (c3 == c2) ++run;
                else { atomicAdd(&s_cnt[c2], run); run = 1; }
                atomicAdd(&s_cnt[c3], run);
            }
        }
        scalar_from = n4 << 2;
    }
    for (long long i = scalar_from + gid; i < n_px; i += stride) {
        const uint8_t *p = rgb + 3 * i;
        atomicAdd(&s_cnt[(((uint32_t)p[0] >> 4) << 8) | (((uint32_t)p[1] >> 4) << 4) | ((uint32_t)p[2] >> 4)], 1u);
    }
    __syncthreads();
    uint32_t *__restrict__ row = sig + (size_t)blockIdx.y * kBins;
    for (int i = threadIdx.x; i < kBins; i += kSigThreads) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(&row[i], c);
    }
}

__global__ __launch_bounds__(kDistThreads) void signature_distance_kernel(const uint32_t *__restrict__ sig, const uint32_t *__restrict__ prev,
                                                                         const int has_prev, long long *__restrict__ dist)
{
    __shared__ unsigned long long s_part[kDistThreads / 64];
    const int i = (int)blockIdx.x, t = (int)threadIdx.x;
    const uint32_t *other = i > 0 ? sig + (size_t)(i - 1) * kBins : (has_prev ? prev : nullptr);   // (uniform over the workgroup)
    if (!other) {
        if (t == 0) dist[0] = 0;
        return;
    }
    const uint4 *a = reinterpret_cast<const uint4 *>(sig + (size_t)i * kBins);
    const uint4 *b = reinterpret_cast<const uint4 *>(other);
    unsigned long long sum = 0ull;
#pragma unroll
    for (int k = 0; k < kBins / 4 / kDistThreads; ++k) {
        const uint4 x = a[k * kDistThreads + t], y = b[k * kDistThreads + t];
        sum += (unsigned long long)(x.x > y.x ? x.x - y.x : y.x - x.x) + (x.y > y.y ? x.y - y.y : y.y - x.y);
        sum += (unsigned long long)(x.z > y.z ? x.z - y.z : y.z - x.z) + (x.w > y.w ? x.w - y.w : y.w - x.w);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((t & 63) == 0) s_part[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long total = 0ull;
#pragma unroll
        for (int w = 0; w < kDistThreads / 64; ++w) total += s_part[w];
        dist[i] = (long long)total;
    }
}

int launch_frame_signatures(const uint8_t *frames, int n_frames, long long n_px, uint32_t *sig, hipStream_t s)
{
    DP_HIP(hipMemsetAsync(sig, 0, (size_t)n_frames * kBins * sizeof(uint32_t), s));
    const long long groups = (n_px + 3) / 4, per_block = (long long)kSigThreads * kSigGroupsPerLane;
    long long bpf = (groups + per_block - 1) / per_block;
    bpf = bpf < 1 ? 1 : (bpf > kSigMaxBlocksPerFrame ? kSigMaxBlocksPerFrame : bpf);
    hipLaunchKernelGGL(frame_signature_kernel, dim3((unsigned)bpf, (unsigned)n_frames), dim3(kSigThreads), 0, s, frames, n_px, sig);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int launch_signature_distances(const uint32_t *sig, int n_frames, uint32_t *prev, int has_prev, long long *dist, hipStream_t s)
{
    hipLaunchKernelGGL(signature_distance_kernel, dim3((unsigned)n_frames), dim3(kDistThreads), 0, s, sig, (const uint32_t *)prev, has_prev, dist);
    DP_HIP(hipGetLastError());
    DP_HIP(hipMemcpyAsync(prev, sig + (size_t)(n_frames - 1) * kBins, kBins * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_frame_signatures_u8(const uint8_t *frames_dev, int n_frames, int h, int w, uint32_t *sig_dev, void *stream)
{
    if (!frames_dev || !sig_dev || ((uintptr_t)sig_dev & 15) || h < 1 || w < 1 || n_frames < 0 || (long long)h * (long long)w >= (1LL << 32)) {
        set_error("dp_frame_signatures_u8: bad argument (h, w >= 1, h * w < 2^32, n_frames >= 0, sig_dev 16-byte aligned)");
        return DP_EINVAL;
    }
    if (n_frames > 65535) {
        set_error("dp_frame_signatures_u8: at most 65535 frames per call, not %d", n_frames);
        return DP_EUNSUPPORTED;
    }
    if (n_frames == 0) return DP_OK;
    return launch_frame_signatures(frames_dev, n_frames, (long long)h * (long long)w, sig_dev, (hipStream_t)stream);
}

int dp_signature_distances(const uint32_t *sig_dev, int n_frames, uint32_t *prev_sig_dev, int has_prev, int64_t *dist_dev, void *stream)
{
    if (!sig_dev || ((uintptr_t)sig_dev & 15) || !prev_sig_dev || ((uintptr_t)prev_sig_dev & 15) || !dist_dev || ((uintptr_t)dist_dev & 7) ||
        n_frames < 0) {
        set_error("dp_signature_distances: bad argument (n_frames >= 0, sig_dev and prev_sig_dev 16-byte, dist_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (n_frames == 0) return DP_OK;
    return launch_signature_distances(sig_dev, n_frames, prev_sig_dev, has_prev ? 1 : 0, reinterpret_cast<long long *>(dist_dev),
                                      (hipStream_t)stream);
}

}  // extern "C"
