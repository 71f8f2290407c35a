/*
 * ditherpie_hip_pattern.h -- pattern (Knoll) dithering with libditherpie_hip.so: an ordered dither for arbitrary palettes.
 * Per pixel a list of n = m * m palette entries whose mean approximates the pixel is built by n nearest-colour searches, the
 * list is sorted by luminance and the m x m Bayer rank matrix picks one of its entries by position alone.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_indexed.h and ditherpie_hip_scene.h are: the test suite pins the device entry points of each header to a
 * memory-discipline matrix; this header has its own (tests/test_gpu_pattern_memory.py) and its own guard
 * (tests/test_pattern_cpu.py).
 *
 * Definition (all integer arithmetic).  For a palette of K <= 256 entries whose pal_f32 values lie in [0, 255]:
 *   C[k]  = trunc(pal_f32[k]) per channel             L[k] = 299 C[k].r + 587 C[k].g + 114 C[k].b
 *   B_m   = the rank matrix: B_2 = [[0, 2], [3, 1]], B_2m = [[4 B, 4 B + 2], [4 B + 3, 4 B + 1]] (a permutation of 0 .. n-1)
 *   nearest(q) = the entry DP_MODE_NEAREST of dp_ordered_u8 assigns to a pixel of colour q with this palette and NO lut_in
 *                (scipy's KD-tree order on ties, not the lowest index)
 * and for the pixel at global position (y, x) = (y0 + row, x0 + column) with source bytes s, c = lut_in[s] (c = s without):
 *   e = (0, 0, 0)
 *   for i in 0 .. n-1:   t = clamp(c + floor(e * strength256 / 256), 0, 255);   k_i = nearest(t);   e += c - C[k_i]
 *   sort the k_i ascending by (L[k], k);   out = out_colors[k_sorted[B_m[y mod m][x mod m]]]
 * strength256 = 0 is DP_MODE_NEAREST itself.  Position-only: frames of a clip get the same pattern, tiles with their global
 * offsets reassemble to the whole image.
 */
#ifndef DITHERPIE_HIP_PATTERN_H
#define DITHERPIE_HIP_PATTERN_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_PATTERN_TABLE_BYTES 16777216 /* one byte per colour of the 2^24 cube */

/* ---- The search table ----
 *
 * The n dependent searches of a pixel are gathers from an exact table of nearest(q) over all 2^24 colours, one byte per
 * colour: the luminance RANK of the entry (its position in the order by (L[k], k)), so that the candidates are directly
 * sortable bytes.  The table is built by running the library's own DP_MODE_NEAREST device path over the identity colours,
 * so it IS that path, tie order included.  It is kept on the dp_palette (16 MiB of device memory per palette that has been
 * used for pattern dithering, freed by dp_palette_destroy) and is built once, lazily, under the palette's build mutex:
 * dp_pattern_prepare builds it ahead of time on the null stream, the first dp_pattern_u8 with the palette builds it on the
 * caller's stream; either waits for the build before it publishes the table to other threads (one device allocation, one
 * small copy in each direction, four nearest-only launches and their fix-up passes: 0.3 ms at 16 colours, 1.3 - 1.7 ms at 256
 * on one MI355X).  Because the build allocates and synchronises, the FIRST dp_pattern_u8 with a palette must not
 * happen while its stream is being captured into a graph: call dp_pattern_prepare before the capture.  Idempotent.
 * DP_EINVAL: a NULL palette.  DP_EUNSUPPORTED: K > 256, a palette value outside [0, 255].
 * dp_pattern_table_bytes: the device memory the table of this palette takes once built (0 for a NULL palette or one that
 * dp_pattern_prepare refuses); no HIP call. */
int dp_pattern_prepare(dp_palette *pal);
size_t dp_pattern_table_bytes(const dp_palette *pal);

/* ---- Pattern dithering ----
 *
 *   in_dev/out_dev  n_frames x h x w x 3 uint8, any address; out_dev may be in_dev itself (a lane reads its pixels before
 *                   it writes them), a partial overlap is not supported
 *   (y0, x0)        global coordinates of pixel (0,0) of every frame (row-band / tile sharding)
 *   matrix          m: 2, 4 or 8
 *   strength256     0 .. 256: the share of the accumulated error that steers the next search, in 1/256
 * One launch per 65535 frames.  n_frames == 0 (with a palette and valid sizes) returns DP_OK without a launch and touches
 * nothing, pointers may then be NULL.
 * DP_EINVAL: a NULL pointer, n_frames < 0, h or w < 1, h * w > 2^30, negative y0 or x0, y0 + h or x0 + w > 2^30, a matrix
 * outside {2, 4, 8}, strength256 outside 0 .. 256.  DP_EUNSUPPORTED: K > 256, a palette value outside [0, 255].
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_pattern_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, int y0, int x0,
                  const dp_palette *pal, int matrix, int strength256, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_PATTERN_H */
