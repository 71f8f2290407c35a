// Integer error diffusion (include/ditherpie_hip_idiff.h): the classical raster scans in sixteenths, the nearest colour by one
// gather from the palette's 2^24-entry table (pattern.hip; for a metric palette the table derived from its top-2 table).
//
// idiff_kernel<PERIOD, NT>  the banded wavefront schedule of ed_band.hip.h on its one-workgroup-per-frame path, minus what the float
//   arithmetic forced on ed_wavefront_kernel (ediff.hip).  One workgroup per frame, up to 16 waves; the bands of the frame go
//   round-robin over the waves; host_logic.h: idiff_plan has the skew.  A wave waits only for the wave that owns the band above,
//   through a progress word in LDS; that wave never waits for it and all waves of a workgroup are resident together, so the wait
//   ends.  Nothing waits across workgroups.
//   Errors: a row's last 8 columns live in a per-row ring in LDS, two words per pixel (r | g << 16, b).  A destination PULLS
//   trunc(e * q_k / 65536) from its finished sources: integer sums, any order, no atomics.  The workspace holds two pairs of
//   boundary rows per frame: band b + 2 overwrites what band b wrote only where band b + 1 is long past (it trails band b + 1 by
//   more than 63 * skew columns, the prefetch looks back 14).  The one global access on the dependency chain is the table gather.
//   The progress word of a wave is band * (w + 1) + (columns of rows 62 / 63 that have landed in the workspace), w columns
//   once the band is finished: it only grows, and band * (w + 1) <= 2^24 + 2^24 as h * w <= 2^30.
//   Taps travel by value.  Instances with 4, 7 and 12 tap slots (the reference's sets have 3, 4, 6, 7, 10 and 12 taps; a
//   spare slot is a tap of share 0): every slot is unconditional, so the LDS reads of a step's taps are all in flight before
//   the first is used -- with one generic instance and a uniform branch per slot each read was waited for in turn, and the
//   32-bit products were quarter-rate v_mad_u64_u32; now they are v_mad_i32_i24 (|e| < 2^12, q <= 2^16).
#include "dp_internal.h"

#include <algorithm>

#include "../../include/ditherpie_hip_idiff.h"
#include "ed_band.hip.h"
#include "pattern_tab.hip.h"

namespace dp {
namespace {

static_assert(kIdiffMaxTaps == DP_IDIFF_MAX_TAPS, "the tap slots of the kernel are the header's limit");
constexpr int kIdMaxWaves = 16;
constexpr int kIdRing = 8;          // per-row ring depth (columns): skew * dy + dx <= 8 for every tap the plan accepts
// Words per row of the ring: 16 are used.  Lane L touches words 2 * ((x - dx) & 7) + {0, 1} of row L with x = t - skew * L; with
// the natural stride of 16 up to eight lanes of a 32-lane half meet in one of the 32 banks of a ds_read2_b32 / ds_write2_b32
// (sixteen at a stride of 20).  17 is conflict-free at skew 2 and at skew 3, for every column phase.
constexpr int kIdRingStride = 17;
constexpr int kIdPeriod = 8;        // steps per I/O period; the experiments build takes 16 with DP_IDIFF_PERIOD=16

__device__ __forceinline__ uint32_t nearest_rank(const PatDev &pd, const uint32_t r, const uint32_t g, const uint32_t b)
{
#ifdef DP_EXPERIMENTS
    if (!pd.brick) return pd.tab[tab_addr<false>(r, g, b)];
#endif
    return pd.tab[tab_addr<true>(r, g, b)];
}

// sign(e) * ((|e| * q) >> 16): the arithmetic shift floors, so a negative e gets 65535 added first.  |e| <= 4080, q <= 65536
__device__ __forceinline__ int share(const int e, const int q) { return (__mul24(e, q) + (int)((uint32_t)e >> 16)) >> 16; }

// the arguments of a MASKED instance behind bnd_all: the mask (n_frames x h x w bytes, non-zero = transparent) and fill (r | g << 8 | b << 16)
__device__ __forceinline__ const uint8_t *id_mask_of(const uint8_t *mask_all, uint32_t) { return mask_all; }
__device__ __forceinline__ uint32_t id_fill_of(const uint8_t *, const uint32_t fill) { return fill; }

// MASK is empty -- the instances of include/ditherpie_hip_idiff.h, whose argument list and code are what they were before the pack
// existed -- or (const uint8_t *, uint32_t): the MASKED instances of include/ditherpie_hip_alpha.h.  There the PERIOD mask bytes of a
// lane's next period travel with its pixel prefetch; a step at a transparent pixel stores zero errors into the ring and into s_bout
// and `fill` into the output bytes, and skips its LDS reads and the gather as a step outside the row does; fences and wave barriers
// stand where they stood.  (mpix, mcur, frame_px, fmask and fill are declared in every instance; an unmasked one never reads them and
// the compiler drops them.)
// Why a pack and not a `bool MASKED` with two trailing arguments: a trailing kernel argument, used or not, moves the hidden arguments
// (the group size the runtime passes behind the explicit ones), which changes an immediate in the unmasked instances; with an empty
// pack their argument list is byte for byte the old one and their gfx950 instruction streams are unchanged (DESIGN.md 4.4 has the
// comparison).  Whoever adds a trailing argument to this kernel moves them for every instance and repeats that comparison.
template <int PERIOD, int NT, typename... MASK>
__global__ __launch_bounds__(64 * kIdMaxWaves) void idiff_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const int h,
                                                                 const int w, const PatDev pd, const uint8_t *__restrict__ lut,
                                                                 const IdiffPlan taps, uint64_t *__restrict__ bnd_all, const MASK... mask_args)
{
    constexpr bool MASKED = sizeof...(MASK) != 0;
    static_assert(sizeof...(MASK) == 0 || sizeof...(MASK) == 2, "no mask arguments, or the mask and the fill");
    constexpr int MW = PERIOD / 4;       // dwords of a period's mask bytes (MASKED)
    constexpr int PW = PERIOD * 3 / 4;   // dwords of a period's pixels
    static_assert(PERIOD % 4 == 0 && PERIOD >= 8 && PERIOD <= 16, "the boundary fetch covers 32 columns per period");
    __shared__ uint32_t s_ring[kIdMaxWaves][64][kIdRingStride];   // errors of the band's own rows: r | g << 16, b
    __shared__ uint32_t s_vring[kIdMaxWaves][2][64][2];           // errors of the two rows above the band (64-column ring)
    __shared__ uint32_t s_bout[kIdMaxWaves][2][PERIOD][2];        // this period's errors of rows 62 / 63, flushed to the workspace
    __shared__ uint32_t s_c[256];                                 // by rank: trunc(pal_f32), r | g<<8 | b<<16
    __shared__ uint32_t s_out[256];                               // by rank: the output bytes
    __shared__ uint8_t s_lut[256];
    __shared__ volatile uint32_t s_prog[kIdMaxWaves];
    __shared__ uint32_t s_zero[2];                                // the "error" of pixels of rows that do not exist
    typedef band_lds_t<uint32_t> lds_u32_t;
    const int L = threadIdx.x & 63, wv = threadIdx.x >> 6, NW = blockDim.x >> 6;
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        s_c[i] = i < pd.K ? pd.c_rank[i] : 0u;
        s_out[i] = i < pd.K ? pd.out_rank[i] : 0u;
        s_lut[i] = lut ? lut[i] : (uint8_t)i;
    }
    if (threadIdx.x < kIdMaxWaves) s_prog[threadIdx.x] = 0u;
    if (threadIdx.x < 2) s_zero[threadIdx.x] = 0u;
    const long frame_bytes = (long)h * w * 3;
    const uint8_t *fin = in + (size_t)blockIdx.x * (size_t)frame_bytes;
    uint8_t *fout = out + (size_t)blockIdx.x * (size_t)frame_bytes;
    uint64_t *bnd = bnd_all + (size_t)blockIdx.x * 4u * (size_t)w;   // [2 buffers][2 rows][w]
    const long frame_px = (long)h * w;
    const uint8_t *__restrict__ fmask = nullptr;
    uint32_t fill = 0u;
    if constexpr (MASKED) {
        fmask = id_mask_of(mask_args...) + (size_t)blockIdx.x * (size_t)frame_px;
        fill = id_fill_of(mask_args...);
    }
    const int skew = taps.skew;
    const int n_bands = (h + 63) / 64;
    const uint32_t w1 = (uint32_t)w + 1u;
    __syncthreads();   // the only workgroup barrier: from here on waves meet through s_prog only

    for (int band = wv; band < n_bands; band += NW) {
        const int r = band * 64 + L;
        const uint64_t *bprev = bnd + (size_t)((band + 1) & 1) * 2u * (size_t)w;   // written by band - 1
        uint64_t *bnext = bnd + (size_t)(band & 1) * 2u * (size_t)w;
        const int rows_here = min(64, h - band * 64);
        const int steps = w + skew * (rows_here - 1);
        const int pw = (wv + NW - 1) % NW;   // the wave that owns band - 1
        const bool row_ok = r < h;
        const long row_byte = (long)r * w * 3;

        // where each tap of this lane's row finds its source row (band_tap_source)
        lds_u32_t *tbase[NT];
        uint32_t tmask[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int dy = taps.dy[k], rel = L - dy;   // (a spare slot: dx = 1, dy = 0, q = 0)
            const bool exists = r - dy >= 0;
            const uint32_t *row = rel >= 0 ? &s_ring[wv][rel][0] : &s_vring[wv][(rel + 2) & 1][0][0];
            band_tap_source<uint32_t>(exists, rel, row, s_zero, kIdRing, tbase[k], tmask[k]);
        }
        uint32_t pix[PW], cur[PW + 1], outb[PW + 1];   // a period's pixels in flight / being consumed / being produced
        uint64_t pb = 0;                               // boundary errors in flight (one column per lane)
        int pb_col = 0;
        bool pb_valid = false;
#pragma unroll
        for (int k = 0; k < PW; ++k) pix[k] = 0;
#pragma unroll
        for (int k = 0; k < PW + 1; ++k) cur[k] = outb[k] = 0;
        uint32_t mpix[MW], mcur[MW];                   // (MASKED) a period's mask bytes in flight / being consumed, one per column
#pragma unroll
        for (int k = 0; k < MW; ++k) mpix[k] = mcur[k] = 0;

        for (int t0 = -PERIOD; t0 < steps + PERIOD; t0 += PERIOD) {
            // ================= period boundary: everything issued one period ago has landed =================
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (L == 0) {
                // the columns of rows 62 / 63 produced in steps < t0 - PERIOD are in the workspace
                const int ack = min(max(t0 - PERIOD - 63 * skew, 0), w);
                s_prog[wv] = (uint32_t)band * w1 + (uint32_t)ack;
            }
            // park the boundary errors fetched during the previous period
            if (pb_valid) {
                uint32_t *dst = &s_vring[wv][L >> 5][pb_col & 63][0];
                dst[0] = (uint32_t)pb;
                dst[1] = (uint32_t)(pb >> 32);
            }
            // ---- flush the outputs of the period that just ended: columns [xs, xs + PERIOD) of row r
            {
                const BandCols c = band_flush<PERIOD>(fout, r, w, (t0 - PERIOD) - skew * L, row_ok, outb);
                if (row_ok && c.hi > c.lo) {
                    // rows 62 / 63: the band's boundary errors of the same period
                    if (L >= 62) {
                        for (int i = c.lo - c.xs; i < c.hi - c.xs; ++i)
                            bnext[(size_t)(L - 62) * (size_t)w + (size_t)(c.xs + i)] =
                                (uint64_t)s_bout[wv][L - 62][i][0] | ((uint64_t)s_bout[wv][L - 62][i][1] << 32);
                    }
                }
            }
            // ---- the pixels fetched during the previous period become current; fetch the next period's
#pragma unroll
            for (int k = 0; k < PW; ++k) cur[k] = pix[k];
            if constexpr (MASKED) {
#pragma unroll
                for (int k = 0; k < MW; ++k) mcur[k] = mpix[k];
            }
            {
                const int xn = (t0 + PERIOD) - skew * L;   // first column of the NEXT period
                const long B = row_byte + (long)xn * 3;
                if (row_ok && xn + PERIOD > 0 && xn < w) {
                    if (B >= 0 && B + 4 * PW <= frame_bytes) {
#pragma unroll
                        for (int k = 0; k < PW; ++k) pix[k] = *reinterpret_cast<const uint32_t *>(fin + B + 4 * k);
                    } else {
#pragma unroll
                        for (int k = 0; k < PW; ++k) {
                            uint32_t v = 0;
#pragma unroll
                            for (int bb = 0; bb < 4; ++bb) {
                                const long a = B + 4 * k + bb;
                                if (a >= 0 && a < frame_bytes) v |= (uint32_t)fin[a] << (8 * bb);
                            }
                            pix[k] = v;
                        }
                    }
                    if constexpr (MASKED) {
                        // the PERIOD mask bytes of the same columns: byte r * w + xn of the frame's mask, at any alignment; bytes in front
                        // of the frame or behind it read as 0 (the columns they stand for are outside the row and never looked at)
                        const long MB = (long)r * w + xn;
                        if (MB >= 0 && MB + 4 * MW <= frame_px) {
#pragma unroll
                            for (int k = 0; k < MW; ++k) mpix[k] = *reinterpret_cast<const uint32_t *>(fmask + MB + 4 * k);
                        } else {
#pragma unroll
                            for (int k = 0; k < MW; ++k) {
                                uint32_t v = 0;
#pragma unroll
                                for (int bb = 0; bb < 4; ++bb) {
                                    const long a = MB + 4 * k + bb;
                                    if (a >= 0 && a < frame_px) v |= (uint32_t)fmask[a] << (8 * bb);
                                }
                                mpix[k] = v;
                            }
                        }
                    }
                }
            }
            // ---- boundary rows of the band above: the 32 columns that end two past lane 0's next period
            pb_valid = false;
            if (band > 0) {
                const int x0n = t0 + PERIOD;              // lane 0's first column of the next period (wave-uniform)
                constexpr int kFirst = PERIOD + 2 - 32;   // (lane 1's taps reach back skew + 2 <= 5 columns)
                const int need = min(x0n + PERIOD + 2, w);   // one past the last column fetched
                if (x0n + kFirst < w && need > 0) {
                    const uint32_t want = (uint32_t)(band - 1) * w1 + (uint32_t)need;
                    while (s_prog[pw] < want) __builtin_amdgcn_s_sleep(4);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    const int col = x0n + kFirst + (L & 31);
                    if (col >= 0 && col < w) {
                        // written by another wave of this workgroup and reused every two bands: bypass L1
                        pb = __hip_atomic_load(bprev + (size_t)(L >> 5) * (size_t)w + (size_t)col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pb_col = col;
                        pb_valid = true;
                    } else if (col >= -2 && col < w + 2) {   // the two columns either side of the image: zero errors
                        pb = 0;
                        pb_col = col;
                        pb_valid = true;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();

            // ================= PERIOD steps that touch LDS, registers and the table only =================
            // four steps per round (band_pixel, band_advance)
            for (int i4 = 0; i4 < PERIOD; i4 += 4) {
                uint32_t cb[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i4 + q;
                    const int x = t0 + i - skew * L;
                    const bool act = row_ok && (uint32_t)x < (uint32_t)w;
                    int e0 = 0, e1 = 0, e2 = 0;
                    uint32_t cbytes = 0;
                    // (MASKED) a transparent pixel takes no part: zero errors go into the ring and into s_bout below, its bytes are `fill`
                    bool live = act;
                    if constexpr (MASKED) {
                        const bool hidden = ((mcur[0] >> (8 * q)) & 255u) != 0u;
                        live = act && !hidden;
                        if (act && hidden) cbytes = fill;
                    }
                    if (live) {
                        const uint32_t pxv = band_pixel(cur, q);
                        uint32_t c0 = pxv & 255u, c1 = (pxv >> 8) & 255u, c2 = (pxv >> 16) & 255u;
                        if (lut) {
                            c0 = s_lut[c0];
                            c1 = s_lut[c1];
                            c2 = s_lut[c2];
                        }
                        // no column test: the rings hold zero errors for the two columns either side of the image (below)
                        // the reads of every tap first, then the sums
                        int a0 = 0, a1 = 0, a2 = 0;
                        uint32_t v0[NT], v1[NT];
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            lds_u32_t *src = tbase[k] + ((x - taps.dx[k]) & (int)tmask[k]) * 2;
                            v0[k] = src[0];
                            v1[k] = src[1];
                        }
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            const int qk = (int)taps.q[k];
                            a0 += share((int)(int16_t)(v0[k] & 0xffffu), qk);
                            a1 += share((int)v0[k] >> 16, qk);
                            a2 += share((int)v1[k], qk);
                        }
                        const int u0 = min(max(16 * (int)c0 + a0, 0), 4080), u1 = min(max(16 * (int)c1 + a1, 0), 4080),
                                  u2 = min(max(16 * (int)c2 + a2, 0), 4080);
                        const uint32_t rk = nearest_rank(pd, (uint32_t)(u0 + 8) >> 4, (uint32_t)(u1 + 8) >> 4, (uint32_t)(u2 + 8) >> 4);
                        const uint32_t cc = s_c[rk];
                        e0 = u0 - 16 * (int)(cc & 255u);
                        e1 = u1 - 16 * (int)((cc >> 8) & 255u);
                        e2 = u2 - 16 * (int)((cc >> 16) & 255u);
                        cbytes = s_out[rk];
                    }
                    cb[q] = cbytes;
                    // every pull of this step precedes the ring writes below (slot x & 7 still holds column x - 8, which a row
                    // below reads in this very step when skew * dy + dx == 8)
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    // columns -2, -1, w and w + 1 are written too, with zero errors: see band_tap_source
                    if (row_ok && x >= -2 && x < w + 2) {
                        uint32_t *slot = &s_ring[wv][L][(x & (kIdRing - 1)) * 2];
                        const uint32_t p0 = ((uint32_t)e0 & 0xffffu) | ((uint32_t)e1 << 16), p1 = (uint32_t)e2;
                        slot[0] = p0;
                        slot[1] = p1;
                        if (act && L >= 62) {
                            s_bout[wv][L - 62][i][0] = p0;
                            s_bout[wv][L - 62][i][1] = p1;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                band_advance<PERIOD>(cur, outb, cb);
                if constexpr (MASKED) {   // the round's four mask bytes are consumed
#pragma unroll
                    for (int k = 0; k < MW - 1; ++k) mcur[k] = mcur[k + 1];
                    mcur[MW - 1] = 0u;
                }
            }
        }
        // band finished: once its boundary stores have landed the band below may read any column
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (L == 0) s_prog[wv] = (uint32_t)band * w1 + (uint32_t)w;
    }
}

}  // namespace

size_t idiff_ws_bytes(const int64_t n_frames, const int h, const int w)
{
    if (n_frames < 0 || h < 1 || w < 1) return 0;
    return (size_t)n_frames * 4u * (size_t)w * sizeof(uint64_t);
}

template <int PERIOD, bool MASKED>
void launch_one(const dim3 grid, const dim3 block, hipStream_t s, const uint8_t *in, uint8_t *out, int h, int w, const PatDev &pd, const uint8_t *lut,
                const IdiffPlan &taps, uint64_t *bnd, const uint8_t *mask, const uint32_t fill)
{
    if constexpr (MASKED) {
        if (taps.n <= 4) hipLaunchKernelGGL((idiff_kernel<PERIOD, 4, const uint8_t *, uint32_t>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd, mask, fill);
        else if (taps.n <= 7) hipLaunchKernelGGL((idiff_kernel<PERIOD, 7, const uint8_t *, uint32_t>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd, mask, fill);
        else hipLaunchKernelGGL((idiff_kernel<PERIOD, kIdiffMaxTaps, const uint8_t *, uint32_t>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd, mask, fill);
    } else {
        if (taps.n <= 4) hipLaunchKernelGGL((idiff_kernel<PERIOD, 4>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd);
        else if (taps.n <= 7) hipLaunchKernelGGL((idiff_kernel<PERIOD, 7>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd);
        else hipLaunchKernelGGL((idiff_kernel<PERIOD, kIdiffMaxTaps>), grid, block, 0, s, in, out, h, w, pd, lut, taps, bnd);
    }
}

// mask: nullptr for the unmasked instances, else n_frames x h x w bytes and the MASKED ones (masked pixels become `fill`)
int launch_idiff(const uint8_t *in, uint8_t *out, int64_t n_frames, int h, int w, const PatDev &pd, const uint8_t *lut, const IdiffPlan &plan,
                 void *ws, hipStream_t s, const uint8_t *mask = nullptr, const uint32_t fill = 0)
{
    IdiffPlan taps = plan;
    for (int k = taps.n; k < kIdiffMaxTaps; ++k) {   // the spare slots of an instance: a tap of the row itself with share 0
        taps.dx[k] = 1;
        taps.dy[k] = 0;
        taps.q[k] = 0;
    }
    const size_t frame = 3 * (size_t)h * (size_t)w;
    const int n_bands = (h + 63) / 64;
    const dim3 block(64 * std::min(kIdMaxWaves, n_bands));
    int period = kIdPeriod;
    if (const char *e = exp_env("DP_IDIFF_PERIOD")) period = std::atoi(e) == 16 ? 16 : 8;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        const uint32_t nf = (uint32_t)std::min<int64_t>(65535, n_frames - f0);
        uint64_t *bnd = reinterpret_cast<uint64_t *>(ws) + (size_t)f0 * 4u * (size_t)w;
        ProfMark *pm = prof_begin(s);
        const uint8_t *fin = in + (size_t)f0 * frame, *fm = mask ? mask + (size_t)f0 * (frame / 3) : nullptr;
        uint8_t *fout = out + (size_t)f0 * frame;
        if (mask && period == 8) launch_one<8, true>(dim3(nf), block, s, fin, fout, h, w, pd, lut, taps, bnd, fm, fill);
        else if (mask) launch_one<16, true>(dim3(nf), block, s, fin, fout, h, w, pd, lut, taps, bnd, fm, fill);
        else if (period == 8) launch_one<8, false>(dim3(nf), block, s, fin, fout, h, w, pd, lut, taps, bnd, nullptr, 0u);
        else launch_one<16, false>(dim3(nf), block, s, fin, fout, h, w, pd, lut, taps, bnd, nullptr, 0u);
        prof_end(pm, s);
        DP_HIP(hipGetLastError());
    }
    return DP_OK;
}

int idiff_call(const char *fn, const bool masked, const uint8_t *in_dev, const uint8_t *mask_dev, const uint32_t fill, uint8_t *out_dev, int64_t n_frames,
               int h, int w, const dp_palette *pal, const int32_t *dx, const int32_t *dy, const int32_t *weight, int n_taps, int divisor, int strength256,
               void *workspace_dev, size_t workspace_bytes, void *stream)
{
    const bool sizes_ok = n_frames >= 0 && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)1 << 30;
    if (!pal || !dx || !dy || !weight || !sizes_ok || (n_frames > 0 && (!in_dev || !out_dev || !workspace_dev || (masked && !mask_dev)))) {
        set_error("%s: bad argument (pointers, n_frames >= 0, h, w >= 1, h * w <= 2^30)", fn);
        return DP_EINVAL;
    }
    IdiffPlan plan;
    static const char *const kRule[] = {"", "a NULL tap array", "n_taps must lie in 1 .. 12", "the divisor must be at least 1",
                                        "strength256 must lie in 0 .. 256", "a tap outside dy 0 .. 2, dx -2 .. 2, dy == 0 with dx >= 1",
                                        "a (dx, dy) given twice", "a negative weight", "weights that sum to more than the divisor"};
    if (const int bad = idiff_plan(dx, dy, weight, n_taps, divisor, strength256, plan)) {
        set_error("%s: %s (n_taps %d, divisor %d, strength256 %d)", fn, kRule[bad], n_taps, divisor, strength256);
        return DP_EINVAL;
    }
    if (in_dev && out_dev == in_dev) {
        set_error("%s: out_dev must not be in_dev", fn);
        return DP_EINVAL;
    }
    if (masked && n_frames > 0) {
        const size_t px = (size_t)n_frames * (size_t)h * (size_t)w;
        const uintptr_t o = (uintptr_t)out_dev, i = (uintptr_t)in_dev, m = (uintptr_t)mask_dev;
        if ((o < i + 3u * px && i < o + 3u * px) || (o < m + px && m < o + 3u * px)) {
            set_error("%s: out_dev must not overlap in_dev or mask_dev", fn);
            return DP_EINVAL;
        }
    }
    if (workspace_dev && ((uintptr_t)workspace_dev & 15u)) {
        set_error("%s: the workspace must be 16-byte aligned", fn);
        return DP_EINVAL;
    }
    int rc = pattern_check_palette(fn, pal);
    if (rc != DP_OK) return rc;
    if (n_frames == 0) return DP_OK;
    if (workspace_bytes < idiff_ws_bytes(n_frames, h, w)) {
        set_error("%s: workspace too small (need %zu bytes)", fn, idiff_ws_bytes(n_frames, h, w));
        return DP_EWORKSPACE;
    }
    rc = pattern_ensure_table(pal, (hipStream_t)stream);
    if (rc != DP_OK) return rc;
    const uint8_t *lut;
    {
        dp_palette *p = const_cast<dp_palette *>(pal);
        std::lock_guard<std::mutex> lock(p->dev_mu);
        lut = p->dev.lut_in;
    }
    return launch_idiff(in_dev, out_dev, n_frames, h, w, pattern_snapshot(pal), lut, plan, workspace_dev, (hipStream_t)stream, masked ? mask_dev : nullptr,
                        fill);
}

}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_idiff_workspace_bytes(int64_t n_frames, int h, int w) { return idiff_ws_bytes(n_frames, h, w); }

int dp_idiff_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, const dp_palette *pal, const int32_t *dx,
                const int32_t *dy, const int32_t *weight, int n_taps, int divisor, int strength256, void *workspace_dev, size_t workspace_bytes,
                void *stream)
{
    return idiff_call("dp_idiff_u8", false, in_dev, nullptr, 0u, out_dev, n_frames, h, w, pal, dx, dy, weight, n_taps, divisor, strength256, workspace_dev,
                      workspace_bytes, stream);
}

}  // extern "C"
