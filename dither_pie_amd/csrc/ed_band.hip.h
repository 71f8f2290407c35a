// The banded wavefront schedule of the raster-scan diffusion kernels, written once: ed_wavefront_kernel (ediff.hip),
// var_wavefront_kernel (vardiff.hip) and idiff_kernel (idiff.hip) call the pieces below from their own band loops.  What differs
// between the families -- ring layout and stride, arithmetic, search, the models, LDS staging of tables -- stays in the kernels.
//
// The schedule.  A wave owns a band of 64 image rows (lane = row) and walks it on the anti-diagonal: lane L works on
// x = t - skew * L at step t, so every source pixel of a row above was finished `skew` steps earlier.  The bands of a frame are
// pipelined across waves: band b + 1 behaves like "lanes 64.." of band b, trailing it by 63 * skew + 3 steps; it spins on a
// progress word that the producing wave publishes after its stores are acknowledged.  Nothing on the dependency chain touches
// global memory (idiff_kernel's table gather apart): all global traffic happens at the boundaries of PERIOD-step periods.  There each
// lane fetches the 3 * PERIOD bytes of its next PERIOD pixels one full period ahead, as unaligned dwords, and flushes the
// output bytes of the period that just ended (band_flush); rows 62 / 63 flush the errors they staged in s_bout during the period to a
// double-buffered row buffer in global memory (L2); and the lanes prefetch, one column each, the 32 columns of the previous band's two
// boundary rows that the next period needs (BandWindow) and park them a period later in a 64-column LDS ring, s_vring -- so every
// wait, one s_waitcnt vmcnt(0) per period, is for operations issued a period earlier.  Errors of the band's own rows live in a
// per-row LDS ring of 8 columns.  Inside a period the waves touch LDS and registers only, ordered by wave-level fences.
// A band follows the one above it at the dependency distance (63 * skew + 2 steps) PLUS three periods of hand-off: its boundary
// errors are stored at the end of their period, acknowledged one period later when the stores have landed, and fetched one period
// before use.  Each kernel has the reason for its period length next to the constant.
#pragma once
#include "dp_internal.h"

namespace dp {
namespace {

template <typename T> using band_lds_t = const __attribute__((address_space(3))) T;

// ---- period output flush and pixel prefetch ---------------------------------------------------------------------------------
// columns [xs, xs + PERIOD) of a lane's row, and the part [lo, hi) of them that lies inside the image
struct BandCols { int xs, lo, hi; };

// The output bytes of the period that just ended, outb[0 .. 3 * PERIOD / 4), go to columns [xs, xs + PERIOD) of row r of the frame:
// whole dwords when the period lies inside the row, byte by byte for the columns inside [0, w) at the two ends of a row.  Then outb
// is cleared.  Returns the columns: the boundary rows flush their errors of the same period next.
template <int PERIOD>
__device__ __forceinline__ BandCols band_flush(uint8_t *fout, const int r, const int w, const int xs, const bool row_ok,
                                               uint32_t (&outb)[PERIOD * 3 / 4 + 1])
{
    constexpr int PW = PERIOD * 3 / 4;
    const int lo = xs < 0 ? 0 : xs, hi = xs + PERIOD > w ? w : xs + PERIOD;
    if (row_ok && hi > lo) {
        const long B = (long)r * w * 3 + (long)xs * 3;
        if (lo == xs && hi == xs + PERIOD) {
#pragma unroll
            for (int k = 0; k < PW; ++k) *reinterpret_cast<uint32_t *>(fout + B + 4 * k) = outb[k];
        } else {
#pragma unroll
            for (int i = 0; i < PERIOD; ++i) {
                if (xs + i >= 0 && xs + i < w) {
                    const int bo = 3 * i;
                    const uint32_t v = __funnelshift_r(outb[bo >> 2], outb[(bo >> 2) + 1], (bo & 3) * 8);
                    uint8_t *o = fout + B + bo;
                    o[0] = (uint8_t)v;
                    o[1] = (uint8_t)(v >> 8);
                    o[2] = (uint8_t)(v >> 16);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PW + 1; ++k) outb[k] = 0;
    return {xs, lo, hi};
}

// NDW dwords at byte offset B of a buffer of `total` bytes: whole (unaligned) dword loads when they stay inside the buffer, else
// assembled bytewise with zeros outside -- the first and the last rows of a frame, whose skewed periods begin before the buffer or
// end past it.  var_wavefront_kernel's pixels of a period (3 * PERIOD / 4 dwords) and its gate bytes (model 3, one per pixel);
// ed_wavefront_kernel and idiff_kernel keep the same fetch written out: through this helper their registers are allocated differently.
template <int NDW>
__device__ __forceinline__ void band_fetch(const uint8_t *buf, const long B, const long total, uint32_t (&dst)[NDW])
{
    if (B >= 0 && B + 4 * NDW <= total) {
#pragma unroll
        for (int k = 0; k < NDW; ++k) dst[k] = *reinterpret_cast<const uint32_t *>(buf + B + 4 * k);
    } else {
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const long a = B + 4 * k + bb;
                if (a >= 0 && a < total) v |= (uint32_t)buf[a] << (8 * bb);
            }
            dst[k] = v;
        }
    }
}

// ---- the steps of a period, in rounds of four: the round's pixels are bytes 0 .. 11 of cur[] and its colours become the LAST twelve
// bytes of outb[] at fixed positions, then both buffers move down by three whole registers (a per-step rotation by three bytes costs
// 24 funnel shifts per step).  The pixel of step q of the round: bytes 3q .. 3q + 2 of the round's twelve
__device__ __forceinline__ uint32_t band_pixel(const uint32_t *cur, const int q)
{
    return q == 0 ? cur[0] : (q == 1 ? __funnelshift_r(cur[0], cur[1], 24) : (q == 2 ? __funnelshift_r(cur[1], cur[2], 16) : (cur[2] >> 8)));
}

// the round's twelve bytes are consumed / produced (cb: the colours of its steps); step i's colour reaches byte 3 * i by the flush
template <int PERIOD>
__device__ __forceinline__ void band_advance(uint32_t (&cur)[PERIOD * 3 / 4 + 1], uint32_t (&outb)[PERIOD * 3 / 4 + 1], const uint32_t (&cb)[4])
{
    constexpr int PW = PERIOD * 3 / 4;
#pragma unroll
    for (int k = 0; k < PW - 3; ++k) {
        cur[k] = cur[k + 3];
        outb[k] = outb[k + 3];
    }
    cur[PW - 3] = cur[PW - 2] = cur[PW - 1] = 0u;
    outb[PW - 3] = cb[0] | (cb[1] << 24);
    outb[PW - 2] = (cb[1] >> 8) | (cb[2] << 16);
    outb[PW - 1] = (cb[2] >> 16) | (cb[3] << 8);
}

// ---- the boundary rows of the band above ----------------------------------------------------------------------------------------
// What a band fetches of them per period: the 32 columns that end two past lane 0's next period, [first(), x0n + PERIOD + 2)
// (lane 1's taps reach back skew + 2 <= 5 columns: PERIOD <= 16).  Lanes 0..31 take row -2 (lane 62 of the band above), lanes 32..63
// row -1 (lane 63), one column each: fetched inside the image, zero errors for the two columns either side of it, else not parked.
// There is something to fetch while first() < w && need > 0.
template <int PERIOD> struct BandWindow {
    static_assert(PERIOD % 4 == 0 && PERIOD >= 4 && PERIOD <= 16, "the boundary fetch covers 32 columns per period");
    static constexpr int kFirst = PERIOD + 2 - 32;
    int x0n;    // lane 0's first column of the next period (wave-uniform)
    int need;   // one past the last column fetched: what the band above must have acknowledged
    __device__ __forceinline__ BandWindow(const int t0, const int w) : x0n(t0 + PERIOD)
    {
        need = x0n + PERIOD + 2;
        need = need > w ? w : need;
    }
    __device__ __forceinline__ int first() const { return x0n + kFirst; }
    __device__ __forceinline__ int col(const int L) const { return x0n + kFirst + (L & 31); }   // lane L's column
};

// ---- where a tap finds its source row -------------------------------------------------------------------------------------------
// The ring of a row of the band (`ring` columns, a power of two), the 64-column ring of the two rows above the band, or -- the row
// does not exist (top of the image), or the slot carries no tap -- the zero slot.  Adding a zero error is exact, so a step needs no
// row test, and no column test either: the rings hold zero errors for the two columns either side of the image.  rel = L - dy: the
// source row relative to the band (-2 .. 63); `row`: that row in its ring, the band's own for rel >= 0
template <typename T>
__device__ __forceinline__ void band_tap_source(const bool exists, const int rel, const T *row, const T *zero, const int ring, band_lds_t<T> *&base,
                                                uint32_t &mask)
{
    base = exists ? (band_lds_t<T> *)row : (band_lds_t<T> *)zero;
    mask = exists ? (rel >= 0 ? (uint32_t)(ring - 1) : 63u) : 0u;
}

// ---- progress words of ed_wavefront_kernel and var_wavefront_kernel --------------------------------------------------------------
// (running band number << 16) | (acknowledged column of row 63 + 1024), one word per wave: s_prog in LDS when the frame has one
// workgroup (G == 1), else agent-scope atomics on the frame's words in global memory -- the workgroups may sit on different XCDs, i.e.
// L2s.  A band waits for the wave that owns the band above until the word says band gb - 1 and a column >= need + 1024, or a later
// band; that loop, with its give-up across workgroups, stands in the two kernels (as a helper it changed their register counts).  (idiff_kernel, one workgroup per frame and no give-up, has a word format of its own.)
constexpr int kBandProgWords = 64;   // progress words per frame in global memory (the last one: the give-up flag)

// inside band gb: the boundary columns produced in steps < t_acked are acknowledged
__device__ __forceinline__ void band_publish(const int G, volatile uint32_t *s_word, uint32_t *g_word, const int gb, const int t_acked, const int skew)
{
    int ack = t_acked - 63 * skew + 1024;
    ack = ack < 0 ? 0 : ack;
    const uint32_t word = ((uint32_t)gb << 16) | (uint32_t)ack;
    if (G == 1) *s_word = word;
    else __hip_atomic_store(g_word, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
}  // namespace dp
