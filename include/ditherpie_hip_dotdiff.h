/*
 * ditherpie_hip_dotdiff.h -- dot diffusion (Knuth 1987) with libditherpie_hip.so: error diffusion without a scan.  Every pixel
 * belongs to a class given by a small tiled class matrix, pixels are quantised in class order and the error of a pixel goes
 * only to its neighbours of a higher class.  Dependencies are local and bounded, so an image is cut into tiles that are
 * diffused independently and exactly.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_pattern.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_dotdiff_memory.py) and its own guard (tests/test_dotdiff_cpu.py).
 *
 * Definition (all integer arithmetic).  The palette conditions are those of ditherpie_hip_pattern.h: K <= 256 entries whose
 * pal_f32 values lie in [0, 255];
 *   C[k]       = trunc(pal_f32[k]) per channel
 *   nearest(q) = the entry DP_MODE_NEAREST of dp_ordered_u8 assigns to a pixel of colour q with this palette and NO lut_in
 *                (scipy's KD-tree order on ties, not the lowest index)
 *   c          = lut_in[s] per channel for the source bytes s of a pixel (c = s without a lut_in)
 * The class matrix M is m x m, m = 2, 4, 8 or 16, a permutation of 0 .. m*m-1; the class of pixel (y, x) is
 * M[y mod m][x mod m].  The eight neighbours of a pixel carry weight 2 (orthogonal) or 1 (diagonal).  Values are kept in
 * sixteenths:
 *   acc = 0 for every pixel and channel
 *   for class = 0 .. m*m-1, for every pixel p of that class (their order does not matter):
 *       v = 16 * c[p] + acc[p]                     per channel
 *       u = clamp(v, 0, 4080)
 *       t = (u + 8) >> 4                           0 .. 255
 *       k = nearest(t);   out[p] = out_colors[k]
 *       e = u - 16 * C[k]
 *       E = the neighbours of p inside the image whose class is GREATER than p's;   W = the sum of their weights
 *       for q in E:   acc[q] += trunc(e * weight(q) * strength256 / (256 * W))     trunc = toward zero, C's '/'
 * strength256 = 0 is DP_MODE_NEAREST itself.  A pixel with an empty E (a "baron") drops its error.  Frames of a batch are
 * independent.  The accumulator fits an int16: a contribution is at most |e| <= 4080 (weight(q) <= W), a pixel receives at
 * most eight, so |acc| <= 32640.
 *
 * Reach.  level(cell) is the largest number of king moves of a path through the periodically tiled matrix that ends in the
 * cell and along which the class strictly increases; reach(M) = the largest level.  Two pixels of equal level are never
 * neighbours, and the output of a pixel depends only on pixels within Chebyshev distance reach(M).  The kernel gives every
 * tile a halo of DP_DOTDIFF_MAX_REACH pixels; a matrix of a larger reach is refused.  (Random 8 x 8 permutations have a
 * median reach of 12, random 16 x 16 ones of 14, the Bayer rank matrices reach 3.)
 *
 * The default matrix of the Python layer, "knuth" (8 x 8, reach 14, barons 62 and 63):
 *   34 48 40 32 29 15 23 31
 *   42 58 56 53 21  5  7 10
 *   50 62 61 45 13  1  2 18
 *   38 46 54 37 25 17  9 26
 *   28 14 22 30 35 49 41 33
 *   20  4  6 11 43 59 57 52
 *   12  0  3 19 51 63 60 44
 *   24 16  8 27 39 47 55 36
 */
#ifndef DITHERPIE_HIP_DOTDIFF_H
#define DITHERPIE_HIP_DOTDIFF_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_DOTDIFF_MAX_REACH 16 /* the halo of a tile: the largest reach of a class matrix that dp_dotdiff_u8 takes */

/* The reach of the m x m class matrix at classes_host (m * m bytes, row-major, host memory), or -1 for a NULL pointer, an m
 * outside {2, 4, 8, 16} or a matrix that is not a permutation of 0 .. m*m-1.  Pure host code: no HIP call, no device. */
int dp_dotdiff_reach(const uint8_t *classes_host, int m);

/* ---- Dot diffusion ----
 *
 *   in_dev/out_dev  n_frames x h x w x 3 uint8, any address.  out_dev must not be in_dev: a tile reads a halo of its
 *                   neighbours' input, so the mode does not work in place; a partial overlap is not supported either
 *   classes_host    the class matrix: m * m bytes of HOST memory, row-major, read during the call (it travels to the kernel
 *                   by value with its level schedule: the call allocates nothing and copies nothing)
 *   strength256     0 .. 256: the share of a pixel's error that is handed on, in 1/256
 * The nearest search is the table of ditherpie_hip_pattern.h, kept on the dp_palette: the first dp_dotdiff_u8 or dp_pattern_u8
 * with a palette builds it on the caller's stream under the palette's build mutex (one device allocation, small copies,
 * the nearest-only launches, a wait for the stream); dp_pattern_prepare builds it ahead of time and serves both modes.
 * Because the build allocates and synchronises, the FIRST call with a palette must not happen while its stream is being
 * captured into a graph: call dp_pattern_prepare before the capture.  With the table in place a call is launches only.
 * One launch per 65535 frames.  n_frames == 0 (with a palette, a matrix and valid sizes) returns DP_OK without a launch and
 * touches nothing, in_dev and out_dev may then be NULL.
 * DP_EINVAL: a NULL pointer, n_frames < 0, h or w < 1, h * w > 2^30, an m outside {2, 4, 8, 16}, a matrix that is not a
 * permutation, strength256 outside 0 .. 256, out_dev == in_dev.  DP_EUNSUPPORTED: K > 256, a palette value outside
 * [0, 255], a matrix whose reach exceeds DP_DOTDIFF_MAX_REACH.
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_dotdiff_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, const dp_palette *pal,
                  const uint8_t *classes_host, int m, int strength256, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_DOTDIFF_H */
