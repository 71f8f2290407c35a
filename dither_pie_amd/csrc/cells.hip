// Cell-palette dithering (include/ditherpie_hip_cells.h): the frame is cut into cw x ch cells, every cell may show k colours
// of its choice (from one of up to four groups) besides the fixed ones; per cell every allowed set is tried on the perturbed
// pixels and the one of least total squared error is taken.
//
// cells_kernel<KSEL>  a workgroup of 256 lanes persists over cells (blockIdx.x, + gridDim.x, ... of frame blockIdx.y).
//   At its start it unranks all candidate masks into LDS (host_logic.h: cells_unrank, the one statement of the enumeration;
//   at most 7280 uint16 = 14.6 KB -- they do not fit kernel arguments and the call must not allocate).  Per cell:
//   1. lane p takes pixel p of the cell (cw * ch <= 256), forms q = clamp(lut[s] + t[y mod m][x mod m]) and writes its K
//      distances into LDS, one COLUMN per palette entry (d(., j) for the pixels of the cell, consecutive lanes consecutive
//      dwords), and the least distance to a FIXED entry into a column of its own.  A pixel beyond the frame writes zeros:
//      it adds nothing to any cost.
//   2. lanes take candidates (rank = lane, + 256, ...).  A lane walks the pixels four at a time: one 16-byte read from each
//      of its KSEL columns, four minima, four additions.  Columns are npx + 4 dwords apart, so column j starts at bank
//      4 j (mod 64): the sixteen columns that the lanes of a wave can address at one step lie in sixteen different 16-byte
//      slots of the 64 banks, equal addresses broadcast -- no conflicts.  cost << 32 | rank, minimised over the wave by
//      shuffles and over the four waves through LDS, is the choice and its tie rule (the candidate enumerated first) at once.
//   3. lane p takes its pixel again and finds the entry of the winning mask with the least distance among its sixteen (ascending
//      j, strict <: the lowest index on ties), then writes its three bytes: byte stores, pixels are 3 bytes at any address
//      and neighbouring cells share dwords.  Lane 0 writes the cell's mask.
//   A cell is read (1) before a barrier and written (3) after it and cells own their bytes: out may be in.
// KSEL (the colours a cell chooses, 1 .. 4) is a template parameter: the reads of a step are straight-line code.
// Measured and replaced (DESIGN.md 4.3f has the figures): one 64-byte ROW per pixel with KSEL dword reads per pixel and
// candidate -- twice the time wherever the search dominates (1820 candidates: 1.01 instead of 0.53 ms per 1080p frame); on
// that layout lut_in staged in LDS, the next cell's bytes loaded a cell ahead and LDS sized per launch changed nothing.
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_cells.h"

namespace dp {
namespace {

constexpr int kCellsBlock = 256;            // lanes of a workgroup = the pixels of the largest cell
constexpr uint32_t kCellsGridTarget = 2048; // workgroups of a launch, about (256 CUs, 5 to 8 each); the rest of the cells by the loop in the kernel
constexpr uint32_t kNoFixed = 0x7fffffffu;  // the fixed column of a pixel when nothing is fixed (never read then)

// what the kernel is given by value
struct CellsDev {
    CellsPlan plan;
    uint32_t c[kCellPalMaxK];   // trunc(pal_f32): r | g<<8 | b<<16
    int8_t t[64];             // the perturbation by (y mod m) * m + (x mod m)
    int K, n_cand, log2m, log2cw, log2ch;
};

template <int KSEL>
__global__ __launch_bounds__(kCellsBlock) void cells_kernel(const uint8_t *in, uint8_t *out, uint16_t *__restrict__ sets, const int h,
                                                            const int w, const uint32_t ncx, const uint32_t ncells, const CellsDev cd,
                                                            const uint32_t *__restrict__ out_rgb, const uint8_t *__restrict__ lut)
{
    __shared__ uint16_t s_mask[kCellPalMaxCandidates];
    __shared__ __attribute__((aligned(16))) uint32_t s_d[kCellPalMaxK * (kCellsBlock + 4)];   // column j: d(p, j) for the pixels p, stride npx + 4
    __shared__ __attribute__((aligned(16))) uint32_t s_fix[kCellsBlock];                  // min over the fixed entries
    __shared__ unsigned long long s_best[kCellsBlock / 64];
    __shared__ int s_t[64];
    static_assert(sizeof(uint16_t) * kCellPalMaxCandidates + sizeof(uint32_t) * (kCellPalMaxK * (kCellsBlock + 4) + kCellsBlock) + 512 <= 32 * 1024,
                  "five workgroups per CU fit its LDS");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_cand = (uint32_t)cd.n_cand, fixed = cd.plan.fixed;
    for (uint32_t r = tid; r < n_cand; r += kCellsBlock) s_mask[r] = (uint16_t)cells_unrank(cd.plan, r);
    if (tid < 64) s_t[tid] = cd.t[tid];

    const int cw = 1 << cd.log2cw, npx = cw << cd.log2ch, mm = (1 << cd.log2m) - 1;
    const int stride = npx + 4;   // dwords between two columns: column j starts at bank 4 j (mod 64) for every npx = 16 .. 256
    const size_t fbase = (size_t)blockIdx.y * 3u * (size_t)h * (size_t)w;
    const uint8_t *fin = in + fbase;
    uint8_t *fout = out + fbase;
    const int py = tid >> cd.log2cw, px = tid & (cw - 1);   // this lane's pixel of a cell (tid < npx)

    for (uint32_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const uint32_t cy = cell / ncx, cx = cell - cy * ncx;
        const int y = (int)(cy << cd.log2ch) + py, x = (int)(cx << cd.log2cw) + px;   // below 2^30 + 16
        const bool inside = tid < npx && y < h && x < w;
        const size_t at = ((size_t)y * (size_t)w + (size_t)x) * 3u;
        __syncthreads();   // the masks are there; the columns of the previous cell are read

        // 1. the distances
        if (tid < npx) {
            uint32_t d[kCellPalMaxK];
            uint32_t fx = kNoFixed;
            if (inside) {
                uint32_t s0 = fin[at], s1 = fin[at + 1], s2 = fin[at + 2];
                if (lut) {
                    s0 = lut[s0];
                    s1 = lut[s1];
                    s2 = lut[s2];
                }
                const int t = s_t[((y & mm) << cd.log2m) | (x & mm)];
                const int q0 = min(max((int)s0 + t, 0), 255), q1 = min(max((int)s1 + t, 0), 255), q2 = min(max((int)s2 + t, 0), 255);
#pragma unroll
                for (int j = 0; j < kCellPalMaxK; ++j) {
                    const uint32_t c = cd.c[j];
                    const int d0 = q0 - (int)(c & 255u), d1 = q1 - (int)((c >> 8) & 255u), d2 = q2 - (int)(c >> 16);
                    d[j] = j < cd.K ? (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2) : 0u;
                    if ((fixed >> j) & 1u) fx = min(fx, d[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < kCellPalMaxK; ++j) d[j] = 0u;
                fx = fixed ? 0u : kNoFixed;
            }
#pragma unroll
            for (int j = 0; j < kCellPalMaxK; ++j) s_d[j * stride + tid] = d[j];   // consecutive lanes, consecutive dwords
            s_fix[tid] = fx;
        }
        __syncthreads();

        // 2. the candidates
        unsigned long long best = ~0ull;
        for (uint32_t r = tid; r < n_cand; r += kCellsBlock) {
            uint32_t left = (uint32_t)s_mask[r] & ~fixed;   // the KSEL chosen entries
            int a[KSEL];
#pragma unroll
            for (int i = 0; i < KSEL; ++i) {
                a[i] = __builtin_ctz(left | 0x10000u);      // (left has KSEL bits; the guard bit only keeps ctz defined)
                left &= left - 1u;
            }
            const uint4 *col[KSEL];
#pragma unroll
            for (int i = 0; i < KSEL; ++i) col[i] = reinterpret_cast<const uint4 *>(&s_d[a[i] * stride]);   // 16-byte aligned: stride % 4 == 0
            const uint4 *fix4 = reinterpret_cast<const uint4 *>(s_fix);
            uint32_t cost = 0u;
            if (fixed) {
#pragma unroll 2
                for (int p4 = 0; p4 < npx / 4; ++p4) {
                    uint4 mn = fix4[p4];
#pragma unroll
                    for (int i = 0; i < KSEL; ++i) {
                        const uint4 v = col[i][p4];
                        mn = make_uint4(min(mn.x, v.x), min(mn.y, v.y), min(mn.z, v.z), min(mn.w, v.w));
                    }
                    cost += (mn.x + mn.y) + (mn.z + mn.w);
                }
            } else {
#pragma unroll 2
                for (int p4 = 0; p4 < npx / 4; ++p4) {
                    uint4 mn = col[0][p4];
#pragma unroll
                    for (int i = 1; i < KSEL; ++i) {
                        const uint4 v = col[i][p4];
                        mn = make_uint4(min(mn.x, v.x), min(mn.y, v.y), min(mn.z, v.z), min(mn.w, v.w));
                    }
                    cost += (mn.x + mn.y) + (mn.z + mn.w);
                }
            }
            const unsigned long long key = ((unsigned long long)cost << 32) | r;   // cost < 2^26
            best = key < best ? key : best;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        best = s_best[0];
#pragma unroll
        for (int i = 1; i < kCellsBlock / 64; ++i) best = s_best[i] < best ? s_best[i] : best;
        const uint32_t S = s_mask[(uint32_t)best];   // (n_cand >= 1: some lane had a candidate)

        // 3. the pixels
        if (inside) {
            uint32_t dmin = 0xffffffffu;
            int jmin = 0;
#pragma unroll
            for (int j = 0; j < kCellPalMaxK; ++j) {
                const uint32_t dj = s_d[j * stride + tid];
                if (((S >> j) & 1u) && dj < dmin) {
                    dmin = dj;
                    jmin = j;
                }
            }
            const uint32_t o = out_rgb[jmin];   // jmin < K: S has no bit at or above K
            fout[at] = (uint8_t)o;
            fout[at + 1] = (uint8_t)(o >> 8);
            fout[at + 2] = (uint8_t)(o >> 16);
        }
        if (sets && tid == 0) sets[(size_t)blockIdx.y * ncells + cell] = (uint16_t)S;
    }
}

int launch_cells(const uint8_t *in, uint8_t *out, uint16_t *sets, int64_t n_frames, int h, int w, int cw, int ch, const CellsDev &cd,
                 const uint32_t *out_rgb, const uint8_t *lut, hipStream_t s)
{
    const size_t frame = 3 * (size_t)h * (size_t)w;
    const uint32_t ncx = ((uint32_t)w + cw - 1) / cw, ncy = ((uint32_t)h + ch - 1) / ch, ncells = ncx * ncy;   // h * w <= 2^30: no overflow
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const uint32_t nf = (uint32_t)std::min<int64_t>(65535, n_frames - f0);
        uint32_t gx = std::max(1u, kCellsGridTarget / nf);
        if (const char *e = exp_env("DP_CELLS_GRID_X")) gx = (uint32_t)std::min(std::max(std::atoi(e), 1), 1 << 20);   // (tests: walk the cell loop)
        gx = std::min(gx, ncells);
        const dim3 grid(gx, nf), block(kCellsBlock);
        uint16_t *sets_f = sets ? sets + (size_t)f0 * ncells : nullptr;
        ProfMark *pm = prof_begin(s);
        switch (cd.plan.colours) {
        case 1: hipLaunchKernelGGL(cells_kernel<1>, grid, block, 0, s, in + (size_t)f0 * frame, out + (size_t)f0 * frame, sets_f, h, w, ncx, ncells, cd, out_rgb, lut); break;
        case 2: hipLaunchKernelGGL(cells_kernel<2>, grid, block, 0, s, in + (size_t)f0 * frame, out + (size_t)f0 * frame, sets_f, h, w, ncx, ncells, cd, out_rgb, lut); break;
        case 3: hipLaunchKernelGGL(cells_kernel<3>, grid, block, 0, s, in + (size_t)f0 * frame, out + (size_t)f0 * frame, sets_f, h, w, ncx, ncells, cd, out_rgb, lut); break;
        default: hipLaunchKernelGGL(cells_kernel<4>, grid, block, 0, s, in + (size_t)f0 * frame, out + (size_t)f0 * frame, sets_f, h, w, ncx, ncells, cd, out_rgb, lut); break;
        }
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

int log2_of(const int v) { return v == 2 ? 1 : (v == 4 ? 2 : (v == 8 ? 3 : 4)); }

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_cells_u8(const uint8_t *in_dev, uint8_t *out_dev, uint16_t *sets_dev, int64_t n_frames, int h, int w, const dp_palette *pal,
                int cw, int ch, int colours, uint32_t fixed_mask, const uint16_t *groups_host, int n_groups, int m, int spread,
                void *stream)
{
    if (metric_refused("dp_cells_u8", pal)) return DP_EUNSUPPORTED;
    const bool sizes_ok = n_frames >= 0 && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)1 << 30;
    if (!pal || !groups_host || !sizes_ok || (n_frames > 0 && (!in_dev || !out_dev))) {
        set_error("dp_cells_u8: bad argument (pointers, n_frames >= 0, h, w >= 1, h * w <= 2^30)");
        return DP_EINVAL;
    }
    if ((cw != 4 && cw != 8 && cw != 16) || (ch != 4 && ch != 8 && ch != 16)) {
        set_error("dp_cells_u8: the cell must be 4, 8 or 16 wide and high, not %d x %d", cw, ch);
        return DP_EINVAL;
    }
    if (m != 2 && m != 4 && m != 8) {
        set_error("dp_cells_u8: the matrix must be 2, 4 or 8, not %d", m);
        return DP_EINVAL;
    }
    if (spread < 0 || spread > 255) {
        set_error("dp_cells_u8: spread must lie in 0 .. 255, not %d", spread);
        return DP_EINVAL;
    }
    if (colours < 1 || colours > kCellPalMaxColours || n_groups < 1 || n_groups > kCellPalMaxGroups) {
        set_error("dp_cells_u8: colours and n_groups must lie in 1 .. 4, not %d and %d", colours, n_groups);
        return DP_EINVAL;
    }
    if ((uintptr_t)sets_dev & 1u) {
        set_error("dp_cells_u8: sets_dev must be 2-byte aligned");
        return DP_EINVAL;
    }
    const int K = pal->dev.K;
    if (K > kCellPalMaxK) {
        set_error("dp_cells_u8: at most 16 colours are supported, the palette has %d", K);
        return DP_EUNSUPPORTED;
    }
    CellsDev cd{};
    cd.n_cand = cells_plan(K, colours, fixed_mask, groups_host, n_groups, cd.plan);
    if (cd.n_cand < 0) {
        set_error("dp_cells_u8: fixed_mask and the groups must name entries below %d, and every group needs %d entries outside "
                  "fixed_mask",
                  K, colours);
        return DP_EINVAL;
    }
    for (const double v : pal->pts_host)
        if (!(v >= 0.0 && v <= 255.0)) {
            set_error("dp_cells_u8: palette values must lie in [0, 255], found %g", v);
            return DP_EUNSUPPORTED;
        }
    if (n_frames == 0) return DP_OK;
    for (int j = 0; j < K; ++j)
        cd.c[j] = (uint32_t)pal->pts_host[3 * j] | ((uint32_t)pal->pts_host[3 * j + 1] << 8) | ((uint32_t)pal->pts_host[3 * j + 2] << 16);
    cells_perturbation(m, spread, cd.t);
    cd.K = K;
    cd.log2m = log2_of(m);
    cd.log2cw = log2_of(cw);
    cd.log2ch = log2_of(ch);
    const uint32_t *out_rgb;
    const uint8_t *lut;
    {
        dp_palette *p = const_cast<dp_palette *>(pal);
        std::lock_guard<std::mutex> lock(p->dev_mu);
        out_rgb = p->dev.out_rgb;
        lut = p->dev.lut_in;
    }
    return launch_cells(in_dev, out_dev, sets_dev, n_frames, h, w, cw, ch, cd, out_rgb, lut, (hipStream_t)stream);
}

}  // extern "C"
