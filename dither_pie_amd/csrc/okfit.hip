// Oklab palette fitting (include/ditherpie_hip_okfit.h): a weighted k-means over the distinct colours of a colour histogram in the
// integer Oklab of metric_lab.hip.h.  Integer sums throughout, so that no result depends on the order of an addition; ties are
// decided by comparing (value, code) or (distance, centre index) as pairs.
//
// POINT RECORDS (16 bytes: code, count, int16 L, a, b, 0), in ascending code = r << 16 | g << 8 | b.
//   okfit_hist_scan_kernel<false>   the histogram is CELL-MAJOR (slot = cell << 12 | r_lo << 8 | g_lo << 4 | b_lo, then the pixels per
//                                   cell), the points are wanted in CODE order: the 16 colours of one (r, g, b_hi) are contiguous in
//                                   both, so a lane owns such a run (64 bytes of counts, four uint4 loads; a run of an empty cell is
//                                   not read at all) and a workgroup the 4096 codes of one (r, g_hi): it counts its occupied colours
//   okfit_block_prefix_kernel       one workgroup: exclusive prefix of the 4096 workgroup counts, and n
//   okfit_hist_scan_kernel<true>    the same scan again; a lane's place is the workgroup's prefix + the lanes before it (a scan in
//                                   LDS); Lab is computed here, once per colour, so that no Lloyd pass takes a cube root
//   okfit_points_kernel             records from (codes, counts) arrays: how tests reach counts near 2^32 and hand-made ties
//
// THE FIT.  Workgroups of 256 lanes (kFitBlock) that stride over the points, a lane one point at a time, with the K centres as
// int4 records in LDS (every lane reads the same entry: a broadcast); the grid is at most kFitMaxBlocks workgroups.
//   okfit_seed_kernel     round r: every workgroup reduces the previous round's partial maxima to centre r - 1 (the same few KB in
//                         every workgroup: no launch of its own for it, workgroup 0 records the centre), folds that centre into dmin
//                         and reduces (count * dmin, lowest index) of its points to one partial.  Partials alternate between two
//                         arrays, a round reads one and writes the other.  Round 0 maximises the count.  K launches, then
//   okfit_seed_last       centre K - 1 from the last partials.  No centre travels through the host.
//   okfit_pass_kernel     one Lloyd pass: brute-force assignment in ascending centre order under a strict comparison (an equal
//                         distance never displaces a lower index), then cnt and S per centre in int64.  When the whole wave agrees on
//                         the centre (points are in code order: neighbours mostly do) the four sums are reduced in the wave and one
//                         lane adds them to LDS; otherwise every lane adds its own (64-bit LDS atomics).  One global atomic per
//                         touched centre and quantity per workgroup.
//   okfit_update_kernel   one workgroup, a lane per centre: (2 S + cnt) / (2 cnt) floored, "did a centre change" in one word, the
//                         totals cleared for the next pass.  The host reads that word.
//   okfit_final_kernel    the assignment once more; per centre the minimum of d << 24 | code over its members (a 64-bit LDS, then
//                         global, atomic minimum: the lowest code on ties falls out of the key) and the distortion
//   okfit_medoid_kernel   a workgroup per centre: a centre without members searches all points; writes the palette bytes and the
//                         centre's coordinates
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_okfit.h"
#include "metric_lab.hip.h"

namespace dp {
namespace {

constexpr int kFitBlock = 256;        // lanes per workgroup = points per workgroup and stride step
constexpr int kFitMaxBlocks = 512;    // workgroups of a fit pass (two per CU): the partial maxima of a seeding round are this many
constexpr int kMaxK = DP_OKFIT_MAX_COLORS;
constexpr size_t kHistTable = (size_t)4 << 24;
constexpr int kScanBlocks = 4096;     // one per (r, g_hi): 4096 codes each

// workspace of the histogram scans: counts of the workgroups | their exclusive prefix and the total
constexpr size_t kScanWsBytes = (size_t)(2 * kScanBlocks + 64) * sizeof(uint32_t);

// workspace of the fit (bytes from its start)
constexpr size_t kOffCentres = 0;                                        // int4 [256]
constexpr size_t kOffTotals = kOffCentres + kMaxK * sizeof(int4);        // uint64 [256][4]: cnt, S_L, S_a, S_b
constexpr size_t kOffKeys = kOffTotals + (size_t)kMaxK * 4 * 8;          // uint64 [256]: d << 24 | code of the medoid
constexpr size_t kOffPartials = kOffKeys + (size_t)kMaxK * 8;            // 2 x kFitMaxBlocks x (uint64 value, uint64 index)
constexpr size_t kOffChanged = kOffPartials + (size_t)2 * kFitMaxBlocks * 16;
constexpr size_t kOffDmin = kOffChanged + 256;                           // uint32 [n]
constexpr unsigned long long kNoKey = ~0ull;

struct Partial {
    unsigned long long value, index;
};

__device__ __forceinline__ void unpack(const uint4 p, int &L, int &A, int &B)
{
    L = (int)(short)(p.z & 0xffffu);
    A = (int)p.z >> 16;
    B = (int)(short)(p.w & 0xffffu);
}

__device__ __forceinline__ uint4 make_point(const uint32_t code, const uint32_t count, const uint16_t *s_lin)
{
    int L, A, B;
    lab_dev<false>(code >> 16, (code >> 8) & 255u, code & 255u, s_lin, nullptr, L, A, B);
    return make_uint4(code, count, ((uint32_t)L & 0xffffu) | ((uint32_t)A << 16), (uint32_t)B & 0xffffu);
}

__device__ __forceinline__ uint32_t dist(const int L, const int A, const int B, const int4 c)
{
    const int x = L - c.x, y = A - c.y, z = B - c.z;
    return (uint32_t)(x * x + y * y + z * z);   // <= 408 098 306
}

// ---------------------------------------------------------------------------------------------------- points
template <bool WRITE>
__global__ __launch_bounds__(256) void okfit_hist_scan_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ cell_count,
                                                              uint32_t *__restrict__ block_count, const uint32_t *__restrict__ block_prefix,
                                                              uint4 *__restrict__ points, const unsigned long long capacity)
{
    __shared__ uint32_t s_wave[4];
    __shared__ uint16_t s_lin[256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    if (WRITE) s_lin[t] = c_lin[t];
    const uint32_t run = blockIdx.x * 256u + t;   // (r, g, b_hi): 2^20 runs of 16 codes
    const uint32_t r = run >> 12, g = (run >> 4) & 255u, bh = run & 15u;
    const uint32_t cell = ((r >> 4) << 8) | ((g >> 4) << 4) | bh;
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = 0u;
    if (cell_count[cell]) {
        const uint4 *src = reinterpret_cast<const uint4 *>(table + (((size_t)cell << 12) | ((r & 15u) << 8) | ((g & 15u) << 4)));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = src[q];
            c[4 * q] = v.x, c[4 * q + 1] = v.y, c[4 * q + 2] = v.z, c[4 * q + 3] = v.w;
        }
    }
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) mine += c[i] != 0u;
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += o;
    }
    if (lane == 63u) s_wave[wv] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        before += w < wv ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    if (!WRITE) {
        if (t == 0) block_count[blockIdx.x] = total;
        return;
    }
    unsigned long long at = (unsigned long long)block_prefix[blockIdx.x] + before + incl - mine;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (c[i] == 0u) continue;
        if (at < capacity) points[at] = make_point((run << 4) | (uint32_t)i, c[i], s_lin);
        ++at;
    }
}

__global__ __launch_bounds__(1024) void okfit_block_prefix_kernel(const uint32_t *__restrict__ block_count, uint32_t *__restrict__ block_prefix,
                                                                  long long *__restrict__ n_out)
{
    __shared__ uint32_t s_part[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t c[4], mine = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[i] = block_count[4 * t + i];
        mine += c[i];
    }
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_part[wv] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;   // at most 2^24
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        before += w < wv ? s_part[w] : 0u;
        total += s_part[w];
    }
    uint32_t at = before + incl - mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        block_prefix[4 * t + i] = at;
        at += c[i];
    }
    if (t == 0) *n_out = (long long)total;
}

__global__ __launch_bounds__(256) void okfit_points_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ counts, const uint32_t n,
                                                           uint4 *__restrict__ points)
{
    __shared__ uint16_t s_lin[256];
    s_lin[threadIdx.x] = c_lin[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) points[i] = make_point(codes[i] & 0xffffffu, counts[i], s_lin);
}

// ---------------------------------------------------------------------------------------------------- seeding
// the greater value, the lower index on equal values
__device__ __forceinline__ bool better(const unsigned long long v, const unsigned long long i, const unsigned long long bv, const unsigned long long bi)
{
    return v > bv || (v == bv && i < bi);
}

// the best (value, index) of the workgroup, in every lane; entries with index kNoKey take part in nothing
__device__ __forceinline__ void block_best(unsigned long long &v, unsigned long long &i, Partial *s_red)
{
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long ov = __shfl_xor(v, m), oi = __shfl_xor(i, m);
        if (oi != kNoKey && (i == kNoKey || better(ov, oi, v, i))) v = ov, i = oi;
    }
    __syncthreads();   // (s_red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = Partial{v, i};
    __syncthreads();
    v = s_red[0].value, i = s_red[0].index;
#pragma unroll
    for (int w = 1; w < kFitBlock / 64; ++w) {
        const Partial o = s_red[w];
        if (o.index != kNoKey && (i == kNoKey || better(o.value, o.index, v, i))) v = o.value, i = o.index;
    }
}

// the centre a finished round chose: the point of the best partial, or centre 0 again when the best product is 0
__device__ __forceinline__ int4 chosen_centre(const Partial *__restrict__ prev, const int n_prev, const int round, const uint4 *__restrict__ points,
                                              const int4 *__restrict__ centres, Partial *s_red)
{
    unsigned long long v = 0ull, i = kNoKey;
    for (int p = threadIdx.x; p < n_prev; p += kFitBlock) {
        const Partial o = prev[p];
        if (i == kNoKey || better(o.value, o.index, v, i)) v = o.value, i = o.index;
    }
    block_best(v, i, s_red);
    if (round > 0 && v == 0ull) return centres[0];   // fewer distinct Labs than centres (round 0 maximises counts: never 0)
    int L, A, B;
    unpack(points[i], L, A, B);
    return make_int4(L, A, B, 0);
}

// round >= 0: partial maxima of round `round` into `mine`; round >= 1 first derives centre round - 1 from `prev` (n_blocks entries)
__global__ __launch_bounds__(kFitBlock) void okfit_seed_kernel(const uint4 *__restrict__ points, const uint32_t n, const int round,
                                                               const Partial *__restrict__ prev, Partial *__restrict__ mine,
                                                               int4 *__restrict__ centres, uint32_t *__restrict__ dmin)
{
    __shared__ Partial s_red[kFitBlock / 64];
    int4 c = make_int4(0, 0, 0, 0);
    if (round > 0) {
        c = chosen_centre(prev, (int)gridDim.x, round - 1, points, centres, s_red);
        if (blockIdx.x == 0 && threadIdx.x == 0) centres[round - 1] = c;
    }
    unsigned long long v = 0ull, at = kNoKey;
    for (uint32_t i = blockIdx.x * kFitBlock + threadIdx.x; i < n; i += gridDim.x * kFitBlock) {
        const uint4 p = points[i];
        unsigned long long val = p.y;
        if (round > 0) {
            int L, A, B;
            unpack(p, L, A, B);
            uint32_t d = dist(L, A, B, c);
            if (round > 1) d = min(d, dmin[i]);   // (round 1 defines dmin: what the workspace held does not matter)
            dmin[i] = d;
            val = (unsigned long long)p.y * d;
        }
        if (at == kNoKey || val > v) v = val, at = i;   // ascending i: an equal value never displaces a lower index
    }
    block_best(v, at, s_red);
    if (threadIdx.x == 0) mine[blockIdx.x] = Partial{v, at};
}

__global__ __launch_bounds__(kFitBlock) void okfit_seed_last(const uint4 *__restrict__ points, const int K, const int n_prev,
                                                             const Partial *__restrict__ prev, int4 *__restrict__ centres)
{
    __shared__ Partial s_red[kFitBlock / 64];
    const int4 c = chosen_centre(prev, n_prev, K - 1, points, centres, s_red);
    if (threadIdx.x == 0) centres[K - 1] = c;
}

// ---------------------------------------------------------------------------------------------------- Lloyd
__device__ __forceinline__ int nearest_centre(const int L, const int A, const int B, const int4 *s_c, const int K, uint32_t &d_out)
{
    uint32_t best = dist(L, A, B, s_c[0]);
    int at = 0;
    for (int k = 1; k < K; ++k) {
        const uint32_t d = dist(L, A, B, s_c[k]);
        if (d < best) best = d, at = k;
    }
    d_out = best;
    return at;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(kFitBlock) void okfit_pass_kernel(const uint4 *__restrict__ points, const uint32_t n, const int K,
                                                               const int4 *__restrict__ centres, unsigned long long *__restrict__ totals)
{
    __shared__ int4 s_c[kMaxK];
    __shared__ unsigned long long s_tot[kMaxK * 4];
    for (int i = threadIdx.x; i < K; i += kFitBlock) s_c[i] = centres[i];
    for (int i = threadIdx.x; i < 4 * K; i += kFitBlock) s_tot[i] = 0ull;
    __syncthreads();
    const uint32_t step = gridDim.x * kFitBlock;
    // (the loop bound is uniform over the wave, so that the ballot below sees every lane; a lane past the end takes no part)
    for (uint32_t base = blockIdx.x * kFitBlock + (threadIdx.x & ~63u); base < n; base += step) {
        const uint32_t i = base + (threadIdx.x & 63u);
        const bool live = i < n;
        int k = -1;
        unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
        if (live) {
            const uint4 p = points[i];
            int L, A, B;
            unpack(p, L, A, B);
            uint32_t d;
            k = nearest_centre(L, A, B, s_c, K, d);
            const long long cnt = (long long)p.y;
            w[0] = p.y;
            w[1] = (unsigned long long)(cnt * L);   // two's complement: the sums wrap to the signed totals
            w[2] = (unsigned long long)(cnt * A);
            w[3] = (unsigned long long)(cnt * B);
        }
        const int k0 = __builtin_amdgcn_readfirstlane(k);
        const bool uniform = __all(k == k0);
        if (uniform && k0 >= 0) {   // every lane is live and agrees: one set of LDS atomics for the wave
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned long long sum = wave_sum(w[q]);
                if ((threadIdx.x & 63u) == 0) atomicAdd(&s_tot[4 * k0 + q], sum);
            }
        } else if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(&s_tot[4 * k + q], w[q]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * K; i += kFitBlock) {
        const unsigned long long v = s_tot[i];
        if (v) atomicAdd(&totals[i], v);
    }
}

__device__ __forceinline__ long long floordiv(const long long a, const long long b)   // b > 0
{
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kMaxK) void okfit_update_kernel(const int K, int4 *__restrict__ centres, unsigned long long *__restrict__ totals,
                                                             uint32_t *__restrict__ changed)
{
    const int k = threadIdx.x;
    int diff = 0;
    if (k < K) {
        const long long cnt = (long long)totals[4 * k];
        if (cnt > 0) {
            const int4 old = centres[k];
            const int4 now = make_int4((int)floordiv(2 * (long long)totals[4 * k + 1] + cnt, 2 * cnt),
                                       (int)floordiv(2 * (long long)totals[4 * k + 2] + cnt, 2 * cnt),
                                       (int)floordiv(2 * (long long)totals[4 * k + 3] + cnt, 2 * cnt), 0);
            diff = now.x != old.x || now.y != old.y || now.z != old.z;
            centres[k] = now;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) totals[4 * k + q] = 0ull;
    }
    const int any = __syncthreads_or(diff);
    if (k == 0) *changed = any ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------------- back to bytes
__global__ __launch_bounds__(kFitBlock) void okfit_final_kernel(const uint4 *__restrict__ points, const uint32_t n, const int K,
                                                                const int4 *__restrict__ centres, unsigned long long *__restrict__ keys,
                                                                unsigned long long *__restrict__ distortion)
{
    __shared__ int4 s_c[kMaxK];
    __shared__ unsigned long long s_key[kMaxK];
    __shared__ unsigned long long s_sum;
    for (int i = threadIdx.x; i < K; i += kFitBlock) {
        s_c[i] = centres[i];
        s_key[i] = kNoKey;
    }
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    unsigned long long sum = 0ull;
    for (uint32_t i = blockIdx.x * kFitBlock + threadIdx.x; i < n; i += gridDim.x * kFitBlock) {
        const uint4 p = points[i];
        int L, A, B;
        unpack(p, L, A, B);
        uint32_t d;
        const int k = nearest_centre(L, A, B, s_c, K, d);
        sum += (unsigned long long)p.y * d;
        atomicMin(&s_key[k], ((unsigned long long)d << 24) | p.x);
    }
    sum = wave_sum(sum);   // (every lane of the wave is here: the loop above has ended for all of them)
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&s_sum, sum);
    __syncthreads();
    for (int i = threadIdx.x; i < K; i += kFitBlock)
        if (s_key[i] != kNoKey) atomicMin(&keys[i], s_key[i]);
    if (threadIdx.x == 0 && s_sum) atomicAdd(distortion, s_sum);
}

__global__ __launch_bounds__(kFitBlock) void okfit_medoid_kernel(const uint4 *__restrict__ points, const uint32_t n, const int4 *__restrict__ centres,
                                                                 const unsigned long long *__restrict__ keys, uint8_t *__restrict__ palette,
                                                                 int32_t *__restrict__ centres_out)
{
    __shared__ unsigned long long s_red[kFitBlock / 64];
    const int k = blockIdx.x;
    const int4 c = centres[k];
    unsigned long long key = keys[k];
    if (key == kNoKey) {   // (uniform over the workgroup) no member: the nearest of all points, the lowest code on ties
        for (uint32_t i = threadIdx.x; i < n; i += kFitBlock) {
            const uint4 p = points[i];
            int L, A, B;
            unpack(p, L, A, B);
            key = min(key, ((unsigned long long)dist(L, A, B, c) << 24) | p.x);
        }
        for (int m = 1; m < 64; m <<= 1) key = min(key, (unsigned long long)__shfl_xor(key, m));
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = key;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kFitBlock / 64; ++w) key = min(key, s_red[w]);
    }
    if (threadIdx.x == 0) {
        const uint32_t code = (uint32_t)key & 0xffffffu;
        palette[3 * k] = (uint8_t)(code >> 16);
        palette[3 * k + 1] = (uint8_t)(code >> 8);
        palette[3 * k + 2] = (uint8_t)code;
        centres_out[3 * k] = c.x;
        centres_out[3 * k + 1] = c.y;
        centres_out[3 * k + 2] = c.z;
    }
}

size_t fit_ws_bytes(const int64_t n) { return kOffDmin + (((size_t)n * sizeof(uint32_t) + 255) & ~(size_t)255); }

int launch_hist_scan(const void *hist, void *points, int64_t capacity, long long *n_out, void *ws, bool write, hipStream_t s)
{
    const uint32_t *table = static_cast<const uint32_t *>(hist);
    const uint32_t *cell_count = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(hist) + kHistTable);
    uint32_t *block_count = static_cast<uint32_t *>(ws), *block_prefix = block_count + kScanBlocks;
    ProfMark *pm = prof_begin(s);
    hipLaunchKernelGGL(okfit_hist_scan_kernel<false>, dim3(kScanBlocks), dim3(256), 0, s, table, cell_count, block_count, nullptr, nullptr, 0ull);
    hipLaunchKernelGGL(okfit_block_prefix_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)block_count, block_prefix, n_out);
    if (write && capacity > 0)
        hipLaunchKernelGGL(okfit_hist_scan_kernel<true>, dim3(kScanBlocks), dim3(256), 0, s, table, cell_count, nullptr, (const uint32_t *)block_prefix,
                           static_cast<uint4 *>(points), (unsigned long long)capacity);
    prof_end(pm, s);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int launch_fit(const void *points_v, int64_t n64, int K, int max_iter, uint8_t *palette, int32_t *centres_out, unsigned long long *distortion,
               int *n_iter_out, void *ws, hipStream_t s)
{
    const uint4 *points = static_cast<const uint4 *>(points_v);
    uint8_t *w = static_cast<uint8_t *>(ws);
    int4 *centres = reinterpret_cast<int4 *>(w + kOffCentres);
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(w + kOffTotals);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w + kOffKeys);
    Partial *partials = reinterpret_cast<Partial *>(w + kOffPartials);
    uint32_t *changed = reinterpret_cast<uint32_t *>(w + kOffChanged);
    uint32_t *dmin = reinterpret_cast<uint32_t *>(w + kOffDmin);
    const uint32_t n = (uint32_t)n64;
    const int blocks = (int)std::min<int64_t>((n64 + kFitBlock - 1) / kFitBlock, kFitMaxBlocks);

    ProfMark *pm = prof_begin(s);   // dp_profile_read: "main" is the seeding, "fix-up" the Lloyd passes (with the host's reads) and the medoids
    DP_HIP(hipMemsetAsync(totals, 0, (size_t)kMaxK * 4 * 8, s));
    DP_HIP(hipMemsetAsync(keys, 0xff, (size_t)kMaxK * 8, s));
    DP_HIP(hipMemsetAsync(distortion, 0, 8, s));
    for (int r = 0; r < K; ++r)
        hipLaunchKernelGGL(okfit_seed_kernel, dim3(blocks), dim3(kFitBlock), 0, s, points, n, r, (const Partial *)(partials + (size_t)((r + 1) & 1) * kFitMaxBlocks),
                           partials + (size_t)(r & 1) * kFitMaxBlocks, centres, dmin);
    hipLaunchKernelGGL(okfit_seed_last, dim3(1), dim3(kFitBlock), 0, s, points, K, blocks, (const Partial *)(partials + (size_t)((K - 1) & 1) * kFitMaxBlocks),
                       centres);
    prof_mid(pm, s);
    DP_HIP(hipGetLastError());
    int n_iter = 0;
    for (int it = 0; it < max_iter; ++it) {
        ++n_iter;
        hipLaunchKernelGGL(okfit_pass_kernel, dim3(blocks), dim3(kFitBlock), 0, s, points, n, K, (const int4 *)centres, totals);
        hipLaunchKernelGGL(okfit_update_kernel, dim3(1), dim3(kMaxK), 0, s, K, centres, totals, changed);
        uint32_t word = 1u;
        DP_HIP(hipMemcpyAsync(&word, changed, sizeof(word), hipMemcpyDeviceToHost, s));
        DP_HIP(hipStreamSynchronize(s));
        if (!word) break;
    }
    hipLaunchKernelGGL(okfit_final_kernel, dim3(blocks), dim3(kFitBlock), 0, s, points, n, K, (const int4 *)centres, keys, distortion);
    hipLaunchKernelGGL(okfit_medoid_kernel, dim3(K), dim3(kFitBlock), 0, s, points, n, (const int4 *)centres, (const unsigned long long *)keys, palette,
                       centres_out);
    prof_end(pm, s);
    DP_HIP(hipGetLastError());
    DP_HIP(hipStreamSynchronize(s));
    *n_iter_out = n_iter;
    return DP_OK;
}

bool misaligned(const void *p, const uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_okfit_hist_workspace_bytes(void) { return kScanWsBytes; }

int dp_okfit_hist_count(const void *hist_dev, int64_t *n_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (!hist_dev || misaligned(hist_dev, 16) || !n_dev || misaligned(n_dev, 8)) {
        set_error("dp_okfit_hist_count: bad argument (hist_dev 16-byte, n_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (!workspace_dev || misaligned(workspace_dev, 16) || workspace_bytes < kScanWsBytes) {
        set_error("dp_okfit_hist_count: workspace too small or not 16-byte aligned (need %zu bytes)", kScanWsBytes);
        return DP_EINVAL;
    }
    return launch_hist_scan(hist_dev, nullptr, 0, reinterpret_cast<long long *>(n_dev), workspace_dev, false, (hipStream_t)stream);
}

int dp_okfit_hist_points(const void *hist_dev, void *points_dev, int64_t capacity, int64_t *n_dev, void *workspace_dev, size_t workspace_bytes,
                         void *stream)
{
    if (!hist_dev || misaligned(hist_dev, 16) || !n_dev || misaligned(n_dev, 8) || capacity < 0 || capacity > DP_OKFIT_MAX_POINTS ||
        (capacity > 0 && (!points_dev || misaligned(points_dev, 16)))) {
        set_error("dp_okfit_hist_points: bad argument (0 <= capacity <= 2^24, hist_dev and points_dev 16-byte, n_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (!workspace_dev || misaligned(workspace_dev, 16) || workspace_bytes < kScanWsBytes) {
        set_error("dp_okfit_hist_points: workspace too small or not 16-byte aligned (need %zu bytes)", kScanWsBytes);
        return DP_EINVAL;
    }
    return launch_hist_scan(hist_dev, points_dev, capacity, reinterpret_cast<long long *>(n_dev), workspace_dev, true, (hipStream_t)stream);
}

int dp_okfit_points_u32(const uint32_t *codes_dev, const uint32_t *counts_dev, int64_t n, void *points_dev, void *stream)
{
    if (n < 0 || n > DP_OKFIT_MAX_POINTS || (n > 0 && (!codes_dev || !counts_dev || !points_dev)) || misaligned(codes_dev, 4) ||
        misaligned(counts_dev, 4) || misaligned(points_dev, 16)) {
        set_error("dp_okfit_points_u32: bad argument (0 <= n <= 2^24, codes_dev and counts_dev 4-byte, points_dev 16-byte aligned)");
        return DP_EINVAL;
    }
    if (n == 0) return DP_OK;
    hipLaunchKernelGGL(okfit_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes_dev, counts_dev, (uint32_t)n,
                       static_cast<uint4 *>(points_dev));
    DP_HIP(hipGetLastError());
    return DP_OK;
}

size_t dp_okfit_workspace_bytes(int64_t n, int K)
{
    if (n < 1 || n > DP_OKFIT_MAX_POINTS || K < 1 || K > DP_OKFIT_MAX_COLORS) return 0;
    return fit_ws_bytes(n);
}

int dp_okfit_fit(const void *points_dev, int64_t n, int K, int max_iter, uint8_t *palette_dev, int32_t *centres_dev, uint64_t *distortion_dev,
                 int *n_iter_out, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (!points_dev || misaligned(points_dev, 16) || n < 1 || n > DP_OKFIT_MAX_POINTS || K < 1 || max_iter < 1 || max_iter > DP_OKFIT_MAX_ITER ||
        !palette_dev || !centres_dev || misaligned(centres_dev, 4) || !distortion_dev || misaligned(distortion_dev, 8) || !n_iter_out) {
        set_error("dp_okfit_fit: bad argument (n >= 1, K >= 1, 1 <= max_iter <= %d, points_dev 16-byte, centres_dev 4-byte, distortion_dev 8-byte aligned)",
                  DP_OKFIT_MAX_ITER);
        return DP_EINVAL;
    }
    if (K > DP_OKFIT_MAX_COLORS) {
        set_error("dp_okfit_fit: at most %d colours are supported, not %d", DP_OKFIT_MAX_COLORS, K);
        return DP_EUNSUPPORTED;
    }
    if (!workspace_dev || misaligned(workspace_dev, 16) || workspace_bytes < fit_ws_bytes(n)) {
        set_error("dp_okfit_fit: workspace too small or not 16-byte aligned (need %zu bytes)", fit_ws_bytes(n));
        return DP_EINVAL;
    }
    return launch_fit(points_dev, n, K, max_iter, palette_dev, centres_dev, reinterpret_cast<unsigned long long *>(distortion_dev), n_iter_out,
                      workspace_dev, (hipStream_t)stream);
}

int dp_okfit_host(const uint32_t *codes, const uint32_t *counts, int64_t n, int K, int max_iter, uint8_t *palette, int32_t *centres, int *n_iter_out,
                  uint64_t *distortion_out)
{
    if (!codes || !counts || !palette || !centres || !n_iter_out || !distortion_out) {
        set_error("dp_okfit_host: bad argument (a null pointer)");
        return DP_EINVAL;
    }
    const int rule = okfit_check(codes, counts, n, K, max_iter);
    if (rule == 2) {
        set_error("dp_okfit_host: at most %d colours are supported, not %d", DP_OKFIT_MAX_COLORS, K);
        return DP_EUNSUPPORTED;
    }
    if (rule) {
        set_error("dp_okfit_host: bad argument (%s)", rule == 1 ? "n >= 1, K >= 1, 1 <= max_iter <= 10000"
                                                      : rule == 3 ? "codes strictly ascending and below 2^24"
                                                                  : "counts >= 1, their sum below 2^32");
        return DP_EINVAL;
    }
    okfit_host(codes, counts, n, K, max_iter, palette, centres, n_iter_out, distortion_out);
    return DP_OK;
}

}  // extern "C"
