// Clip-wide palettes (include/ditherpie_hip_clip.h): the C entry points of the stream form of the distinct-colour passes
// (the kernels are distinct.hip's, STREAM instances) and the rank sample of a colour histogram.
//
// Rank sample.  A histogram of dp_kmeans_hist_build_u8 is count[slot] over 2^24 slots in CELL-MAJOR order (slot = cell << 12 |
// r_lo << 8 | g_lo << 4 | b_lo, cell = r_hi << 8 | g_hi << 4 | b_hi) followed by the pixels per cell.  Laid out in slot order,
// every colour count times, its pixels have ranks 0 .. total - 1; the pixel of rank k is found by
//   cell_prefix_kernel   one workgroup: exclusive 64-bit prefix sum of the 4096 per-cell totals (32 KB, in the workspace) + the total
//   rank_sample_kernel   one wave per rank: binary search of the prefix for the cell (12 steps over 32 KB, L2), then the cell's
//                        16 KB slice in 16 chunks of 256 counts -- a uint4 per lane, an inclusive wave scan of the lane sums --
//                        until the chunk that holds the rank, the lane inside it, the count inside the lane.
// 16 KB read per rank at most (10 000 ranks: 160 MB, against 64 MB x 10 000 for a scan of the table); integers throughout.
#include "dp_internal.h"

#include "../../include/ditherpie_hip_clip.h"

namespace dp {
namespace {

constexpr int kCells = 4096;
constexpr size_t kTableBytes = (size_t)4 << 24;
constexpr size_t kPrefixBytes = (size_t)(kCells + 1) * sizeof(unsigned long long);
constexpr int kSampleWaves = 4;   // ranks per workgroup

__global__ __launch_bounds__(1024) void cell_prefix_kernel(const uint32_t *__restrict__ cell_count, unsigned long long *__restrict__ prefix)
{
    __shared__ unsigned long long s_part[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    unsigned long long c[4], mine = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[i] = cell_count[4 * t + i];
        mine += c[i];
    }
    unsigned long long incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_part[wv] = incl;
    __syncthreads();
    unsigned long long before = 0ull, total = 0ull;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        before += w < wv ? s_part[w] : 0ull;
        total += s_part[w];
    }
    unsigned long long at = before + incl - mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        prefix[4 * t + i] = at;
        at += c[i];
    }
    if (t == 0) prefix[kCells] = total;
}

__global__ __launch_bounds__(64 * kSampleWaves) void rank_sample_kernel(const uint32_t *__restrict__ table, const unsigned long long *__restrict__ prefix,
                                                                        const long long *__restrict__ ranks, const int n_ranks,
                                                                        uint8_t *__restrict__ out, unsigned long long *__restrict__ n_bad)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kSampleWaves + (threadIdx.x >> 6);
    if (i >= n_ranks) return;   // (wave-uniform)
    const long long rank = ranks[i];
    const unsigned long long total = prefix[kCells];
    uint32_t colour = 0u;
    bool found = false;
    if (rank >= 0 && (unsigned long long)rank < total) {
        const unsigned long long k = (unsigned long long)rank;
        // the last cell whose prefix is <= k (empty cells share their successor's prefix and are skipped by "last")
        int lo = 0, hi = kCells - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (prefix[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        const int cell = lo;
        unsigned long long left = k - prefix[cell];   // rank inside the cell
        const uint4 *slice = reinterpret_cast<const uint4 *>(table + ((size_t)cell << 12));
#pragma unroll 1
        for (int chunk = 0; chunk < 16 && !found; ++chunk) {
            const uint4 v = slice[chunk * 64 + lane];
            const unsigned long long mine = (unsigned long long)v.x + v.y + v.z + v.w;
            unsigned long long incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            const unsigned long long chunk_total = __shfl(incl, 63);
            if (left < chunk_total) {   // (wave-uniform)
                const unsigned long long owner = __ballot(left < incl);   // the first lane whose inclusive sum passes the rank
                const int src = __ffsll((long long)owner) - 1;
                uint32_t lo12 = 0u;
                if (lane == src) {
                    unsigned long long r = left - (incl - mine);
                    const uint32_t cnt[4] = {v.x, v.y, v.z, v.w};
                    int q = 0;
                    while (q < 3 && r >= cnt[q]) {
                        r -= cnt[q];
                        ++q;
                    }
                    lo12 = (uint32_t)(chunk * 256 + lane * 4 + q);
                }
                lo12 = (uint32_t)__shfl((int)lo12, src);
                const uint32_t c = (uint32_t)cell;
                const uint32_t r8 = ((c >> 8) << 4) | (lo12 >> 8), g8 = (((c >> 4) & 15u) << 4) | ((lo12 >> 4) & 15u), b8 = ((c & 15u) << 4) | (lo12 & 15u);
                colour = r8 | (g8 << 8) | (b8 << 16);
                found = true;
            } else {
                left -= chunk_total;
            }
        }
    }
    if (lane == 0) {
        out[(size_t)i * 3 + 0] = (uint8_t)colour;
        out[(size_t)i * 3 + 1] = (uint8_t)(colour >> 8);
        out[(size_t)i * 3 + 2] = (uint8_t)(colour >> 16);
        if (!found) atomicAdd(n_bad, 1ull);   // out of range (or a histogram whose cell totals disagree with its counts)
    }
}

}  // namespace

size_t hist_sample_ws_bytes() { return (kPrefixBytes + 255) & ~(size_t)255; }

int launch_hist_sample(const void *hist, const long long *ranks, int n_ranks, uint8_t *out, unsigned long long *n_bad, void *ws, hipStream_t s)
{
    const uint32_t *table = static_cast<const uint32_t *>(hist);
    const uint32_t *cell_count = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(hist) + kTableBytes);
    unsigned long long *prefix = static_cast<unsigned long long *>(ws);
    hipLaunchKernelGGL(cell_prefix_kernel, dim3(1), dim3(1024), 0, s, cell_count, prefix);
    hipLaunchKernelGGL(rank_sample_kernel, dim3((unsigned)((n_ranks + kSampleWaves - 1) / kSampleWaves)), dim3(64 * kSampleWaves), 0, s, table,
                       (const unsigned long long *)prefix, ranks, n_ranks, out, n_bad);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_distinct_stream_state_bytes(void) { return distinct_stream_state_bytes(); }

size_t dp_distinct_stream_workspace_bytes(int64_t n) { return n < 0 ? 0 : distinct_stream_ws_bytes(n); }

int dp_distinct_stream_reset(void *state_dev, int64_t *n_distinct_dev, void *stream)
{
    if (!state_dev || ((uintptr_t)state_dev & 15) || !n_distinct_dev || ((uintptr_t)n_distinct_dev & 7)) {
        set_error("dp_distinct_stream_reset: bad argument (state_dev 16-byte, n_distinct_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    return launch_distinct_stream_reset(state_dev, reinterpret_cast<long long *>(n_distinct_dev), (hipStream_t)stream);
}

int dp_distinct_stream_add_u8(const uint8_t *px_dev, int64_t n, void *state_dev, uint8_t *list_dev, int64_t *n_distinct_dev,
                              void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if ((!px_dev && n > 0) || n < 0 || n > (int64_t)0xfffffff0LL || !state_dev || ((uintptr_t)state_dev & 15) || !list_dev || !n_distinct_dev ||
        ((uintptr_t)n_distinct_dev & 7)) {
        set_error("dp_distinct_stream_add_u8: bad argument (n must be below 2^32 - 16, state_dev 16-byte, n_distinct_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (n == 0) return DP_OK;
    if (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < distinct_stream_ws_bytes(n)) {
        set_error("dp_distinct_stream_add_u8: workspace too small or not 16-byte aligned (need %zu bytes)", distinct_stream_ws_bytes(n));
        return DP_EINVAL;
    }
    return launch_distinct_stream_add(px_dev, n, state_dev, list_dev, reinterpret_cast<long long *>(n_distinct_dev), workspace_dev,
                                      (hipStream_t)stream);
}

size_t dp_hist_sample_workspace_bytes(void) { return hist_sample_ws_bytes(); }

int dp_hist_sample_u8(const void *hist_dev, const int64_t *ranks_dev, int n_ranks, uint8_t *out_dev, int64_t *n_out_of_range_dev,
                      void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (!hist_dev || ((uintptr_t)hist_dev & 15) || n_ranks < 0 || n_ranks > 16384 || !n_out_of_range_dev || ((uintptr_t)n_out_of_range_dev & 7) ||
        (n_ranks > 0 && (!ranks_dev || ((uintptr_t)ranks_dev & 7) || !out_dev))) {
        set_error("dp_hist_sample_u8: bad argument (0 <= n_ranks <= 16384, hist_dev 16-byte, ranks_dev and n_out_of_range_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (n_ranks == 0) return DP_OK;
    if (!workspace_dev || ((uintptr_t)workspace_dev & 15) || workspace_bytes < hist_sample_ws_bytes()) {
        set_error("dp_hist_sample_u8: workspace too small or not 16-byte aligned (need %zu bytes)", hist_sample_ws_bytes());
        return DP_EINVAL;
    }
    return launch_hist_sample(hist_dev, reinterpret_cast<const long long *>(ranks_dev), n_ranks, out_dev,
                              reinterpret_cast<unsigned long long *>(n_out_of_range_dev), workspace_dev, (hipStream_t)stream);
}

}  // extern "C"
