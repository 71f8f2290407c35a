// Void-and-cluster rank matrices (include/ditherpie_hip_voidcluster.h) on the device; the statement is host_logic.h: vac_generate.
//
// One workgroup of 1024 lanes per matrix, steps 2 to 5 in one launch.  Lane t owns the cells p = t + 1024 k (up to 16 at
// 128 x 128): their energies live in LDS (64 KB at 128 x 128), their set bits in one register of the owner.  The seed
// pattern and the prototype are bitmasks in LDS, written with one ballot per 64 cells; the energy of a whole pattern is
// gathered from such a mask (after step 4 the energy is exactly zero, so the prototype needs no copy of it).
// A round is one fused pass: every lane adds or subtracts the weight of the cell just flipped where the minimum-image
// distance is within the weights' reach -- a test per cell, no loop over offsets, so a window wider than the matrix still
// touches every cell once -- and takes the next extremum over its cells as one uint64 (value << 32 | cell): the smallest key
// is the smallest energy and then the lowest cell; the largest energy is the smallest 0x7fffffff - energy.  The keys are
// reduced across the wave with ds_bpermute butterflies and across the 16 waves through 17 LDS words, two barriers a pass.
#include "dp_internal.h"
#include "wave_util.hip.h"

namespace dp {
namespace {

constexpr int kVacThreads = 1024;
constexpr int kVacWaves = kVacThreads / 64;
constexpr int kVacMaxCells = kVacMaxSize * kVacMaxSize;
constexpr int kVacBatch = 64;   // matrices per launch: their seeds travel by value

struct VacDev {
    int32_t wt[kVacMaxWeights];
    uint32_t seeds[kVacBatch];
    int D, h, w;
};

constexpr uint64_t kNoCell = ~0ull;

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t k)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = ((uint64_t)lane_xor_u32((uint32_t)(k >> 32), off) << 32) | lane_xor_u32((uint32_t)k, off);
        k = o < k ? o : k;
    }
    return k;
}

struct VacBlock {
    int32_t *E;            // n energies
    const int32_t *W;      // D + 1 weights
    uint64_t *part;        // kVacWaves + 1 words: the waves' minima, then the workgroup's
    uint32_t *cnt;         // kVacWaves + 1 words: the same for counts
    int n, h, w, D, tid;
    int y0, x0, sy, sx;    // the lane's first cell and the step to its next one (1024 cells on)
    uint32_t on;           // bit k: cell tid + 1024 k is set

    // the smallest key of the workgroup, to every lane
    __device__ uint64_t block_min(uint64_t k) const
    {
        k = wave_min_u64(k);
        if ((tid & 63) == 0) part[tid >> 6] = k;
        __syncthreads();
        if (tid < 64) {
            uint64_t b = tid < kVacWaves ? part[tid] : kNoCell;
            for (int off = kVacWaves / 2; off >= 1; off >>= 1) {
                const uint64_t o = ((uint64_t)lane_xor_u32((uint32_t)(b >> 32), off) << 32) | lane_xor_u32((uint32_t)b, off);
                b = o < b ? o : b;
            }
            if (tid == 0) part[kVacWaves] = b;
        }
        __syncthreads();
        return part[kVacWaves];
    }

    __device__ uint32_t block_sum(uint32_t v) const
    {
        for (int off = 32; off >= 1; off >>= 1) v += lane_xor_u32(v, off);
        if ((tid & 63) == 0) cnt[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            uint32_t s = 0;
            for (int i = 0; i < kVacWaves; ++i) s += cnt[i];
            cnt[kVacWaves] = s;
        }
        __syncthreads();
        return cnt[kVacWaves];
    }

    // One round: flip cell q (sign +1 sets it, -1 clears it, 0: no flip) and return the next extremum -- over the set cells
    // the largest energy (want_set), over the others the smallest; the lowest cell on ties; -1 when there is no such cell.
    __device__ int pass(const int q, const int sign, const bool want_set)
    {
        int qy = 0, qx = 0;
        if (sign) {
            qy = q / w;
            qx = q - qy * w;
        }
        uint64_t best = kNoCell;
        int y = y0, x = x0;
        for (int k = 0, p = tid; p < n; ++k, p += kVacThreads) {
            int32_t e = E[p];
            if (sign) {
                const int d2 = vac_d2(y, x, qy, qx, h, w);
                if (d2 <= D) {
                    e += sign * W[d2];
                    E[p] = e;
                }
                if (p == q) on ^= 1u << k;
            }
            if ((((on >> k) & 1u) != 0u) == want_set) {
                const uint64_t key = ((uint64_t)(uint32_t)(want_set ? 0x7fffffff - e : e) << 32) | (uint32_t)p;
                best = key < best ? key : best;
            }
            x += sx;
            y += sy;
            if (x >= w) {
                x -= w;
                ++y;
            }
        }
        const uint64_t r = block_min(best);
        return r == kNoCell ? -1 : (int)(uint32_t)r;
    }

    // mask (ceil(n / 32) words) = the set bits of every lane; visible after the next barrier
    __device__ void publish(uint32_t *mask) const
    {
        const int rounds = (n + kVacThreads - 1) / kVacThreads;   // the same for every lane: a ballot needs the whole wave
        for (int k = 0; k < rounds; ++k) {
            const int p = tid + kVacThreads * k;
            const uint64_t b = __ballot(p < n && ((on >> k) & 1u));
            if ((tid & 63) == 0 && p < n) {
                mask[p >> 5] = (uint32_t)b;
                if (p + 32 < n) mask[(p >> 5) + 1] = (uint32_t)(b >> 32);
            }
        }
    }

    // the pattern of mask: the lanes' set bits and, from nothing, the energy of every cell.  A lane touches its own cells
    // only, so the set cells are walked without a barrier between them.
    __device__ void adopt(const uint32_t *mask)
    {
        on = 0u;
        for (int k = 0, p = tid; p < n; ++k, p += kVacThreads) {
            on |= ((mask[p >> 5] >> (p & 31)) & 1u) << k;
            E[p] = 0;
        }
        for (int wi = 0; wi < (n + 31) / 32; ++wi)
            for (uint32_t bits = mask[wi]; bits; bits &= bits - 1u) {
                const int q = wi * 32 + __ffs((int)bits) - 1, qy = q / w, qx = q - qy * w;
                int y = y0, x = x0;
                for (int p = tid; p < n; p += kVacThreads) {
                    const int d2 = vac_d2(y, x, qy, qx, h, w);
                    if (d2 <= D) E[p] += W[d2];
                    x += sx;
                    y += sy;
                    if (x >= w) {
                        x -= w;
                        ++y;
                    }
                }
            }
    }
};

__global__ __launch_bounds__(kVacThreads) void void_cluster_kernel(uint16_t *__restrict__ ranks_all, const VacDev a)
{
    __shared__ int32_t s_E[kVacMaxCells];
    __shared__ int32_t s_W[kVacMaxWeights];
    __shared__ uint32_t s_mask[kVacMaxCells / 32];
    __shared__ uint64_t s_part[kVacWaves + 1];
    __shared__ uint32_t s_cnt[kVacWaves + 1];

    VacBlock B;
    B.E = s_E;
    B.W = s_W;
    B.part = s_part;
    B.cnt = s_cnt;
    B.h = a.h;
    B.w = a.w;
    B.D = a.D;
    B.n = a.h * a.w;
    B.tid = (int)threadIdx.x;
    B.y0 = B.tid / a.w;
    B.x0 = B.tid - B.y0 * a.w;
    B.sy = kVacThreads / a.w;
    B.sx = kVacThreads - B.sy * a.w;
    B.on = 0u;
    const int n = B.n, tid = B.tid;
    const uint32_t seed = a.seeds[blockIdx.x];
    uint16_t *__restrict__ ranks = ranks_all + (size_t)blockIdx.x * (size_t)n;

    for (int i = tid; i <= a.D; i += kVacThreads) s_W[i] = a.wt[i];

    // step 2: the n1 cells of the smallest key.  The keys of distinct cells differ (vac_key), so the pattern is key <= the
    // n1-th smallest key, found bit by bit from the top: a bit is set when fewer than n1 keys lie below the candidate.
    const int n1 = max(1, n / 10);
    uint32_t last = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = last | (1u << bit);
        uint32_t below = 0u;
        for (int p = tid; p < n; p += kVacThreads) below += vac_key((uint32_t)p, seed) < cand ? 1u : 0u;
        if (B.block_sum(below) < (uint32_t)n1) last = cand;
    }
    for (int k = 0, p = tid; p < n; ++k, p += kVacThreads) B.on |= (vac_key((uint32_t)p, seed) <= last ? 1u : 0u) << k;
    B.publish(s_mask);
    __syncthreads();   // (also: s_W is complete)
    B.adopt(s_mask);

    // step 3.  The pass that sets v already looks for the next round's c; after the last round that is step 4's first cell.
    int c = B.pass(-1, 0, true);
    for (int round = 0;;) {
        const int v = B.pass(c, -1, false);
        const bool same = v == c;
        c = B.pass(v, +1, true);
        if (same || ++round >= 4 * n) break;
    }
    B.publish(s_mask);   // the prototype; every pass below ends in barriers

    // step 4
    for (int r = n1 - 1; r >= 0; --r) {
        if (tid == 0 && c >= 0) ranks[c] = (uint16_t)r;   // (r + 1 cells are set: there is a c)
        c = B.pass(c, -1, true);
    }

    // step 5, from the prototype
    B.adopt(s_mask);
    int v = B.pass(-1, 0, false);
    for (int r = n1; r < n; ++r) {
        if (tid == 0 && v >= 0) ranks[v] = (uint16_t)r;   // (n - r cells are unset: there is a v)
        if (r + 1 < n) v = B.pass(v, +1, false);
    }
}

}  // namespace

int launch_void_cluster(uint16_t *ranks_dev, int n_matrices, const uint32_t *seeds_host, int h, int w, int sigma256, hipStream_t s)
{
    VacDev a;
    VacWeights W;
    vac_weights(sigma256, W);
    for (int i = 0; i < kVacMaxWeights; ++i) a.wt[i] = W.w[i];
    a.D = W.D;
    a.h = h;
    a.w = w;
    for (int m0 = 0; m0 < n_matrices; m0 += kVacBatch) {
        const int nb = std::min(kVacBatch, n_matrices - m0);
        for (int i = 0; i < kVacBatch; ++i) a.seeds[i] = i < nb ? seeds_host[m0 + i] : 0u;
        ProfMark *pm = prof_begin(s);
        hipLaunchKernelGGL(void_cluster_kernel, dim3(nb), dim3(kVacThreads), 0, s, ranks_dev + (size_t)m0 * (size_t)h * (size_t)w, a);
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

}  // namespace dp

using namespace dp;

extern "C" {

int dp_void_cluster_u16(uint16_t *ranks_dev, int n_matrices, const uint32_t *seeds_host, int h, int w, int sigma256, void *stream)
{
    if (n_matrices < 0 || (n_matrices > 0 && (!ranks_dev || !seeds_host))) {
        set_error("dp_void_cluster_u16: bad argument (pointers, n_matrices >= 0)");
        return DP_EINVAL;
    }
    if (!vac_args_ok(h, w, sigma256)) {
        set_error("dp_void_cluster_u16: h and w must lie in %d .. %d and sigma256 in %d .. %d, not %d x %d and %d", kVacMinSize, kVacMaxSize,
                  kVacMinSigma256, kVacMaxSigma256, h, w, sigma256);
        return DP_EINVAL;
    }
    if (n_matrices == 0) return DP_OK;
    return launch_void_cluster(ranks_dev, n_matrices, seeds_host, h, w, sigma256, (hipStream_t)stream);
}

}  // extern "C"
