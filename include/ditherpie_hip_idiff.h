/*
 * ditherpie_hip_idiff.h -- integer error diffusion with libditherpie_hip.so: the classical raster scans (Floyd-Steinberg,
 * Jarvis-Judice-Ninke, Stucki, Burkes, Atkinson, the Sierras, or any tap set of that shape) in integer arithmetic, with the
 * nearest colour taken from the palette's exact 2^24-entry table.  The search is one gather whatever the palette size, and
 * because the table serves either colour metric, this is the scan that takes a palette of DP_METRIC_OKLAB.
 * dp_error_diffusion_u8 stays what it is: bit-identical to the reference's float scan, RGB palettes only.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_dotdiff.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_idiff_memory.py) and its own guard (tests/test_idiff_cpu.py).
 *
 * Definition (all integer arithmetic, values in sixteenths; tests/idiff_ref.py states it in numpy).  The palette conditions
 * are those of ditherpie_hip_pattern.h: K <= 256 entries whose pal_f32 values lie in [0, 255];
 *   C[k]       = trunc(pal_f32[k]) per channel
 *   nearest(q) = the entry DP_MODE_NEAREST assigns to a pixel of colour q with this palette and NO lut_in: scipy's KD-tree
 *                order on ties for an RGB palette, the metric's nearest (lowest index on ties) for a metric palette -- the
 *                nearest of ditherpie_hip_dotdiff.h
 *   c          = lut_in[s] per channel for the source bytes s of a pixel (c = s without a lut_in)
 * Taps: n_taps triples (dx, dy, weight) and a divisor, int32, in host arrays, with 1 <= n_taps <= 12, dy in 0 .. 2, dx in
 * -2 .. 2, dy == 0 only with dx >= 1, no (dx, dy) twice, weights >= 0, divisor >= 1, sum of the weights <= divisor (the
 * reference's eight tap sets qualify), and
 *   q_k = floor(weight_k * strength256 * 256 / divisor),   strength256 in 0 .. 256
 * so that sum q_k <= 65536: the error is never amplified.  The scan is the plain raster, no serpentine:
 *   acc = 0 for every pixel and channel
 *   for y = 0 .. h-1, for x = 0 .. w-1:
 *       v = 16 * c[y][x] + acc[y][x]               per channel
 *       u = clamp(v, 0, 4080)
 *       t = (u + 8) >> 4                           0 .. 255
 *       k = nearest(t);   out[y][x] = out_colors[k]
 *       e = u - 16 * C[k]                          |e| <= 4080
 *       for each tap with (y + dy, x + dx) inside the image:
 *           acc[y + dy][x + dx] += sign(e) * ((|e| * q_k) >> 16)      trunc toward zero, no division; |e| * q_k < 2^28
 * A pixel receives at most one contribution per tap, so |acc| <= 4080 * sum q_k / 65536 <= 4080: an int16.  Each
 * contribution is truncated on its own and the sums are integer, so every order of the additions gives the same result, push
 * or pull.  strength256 = 0 is DP_MODE_NEAREST itself.  Frames of a batch are independent.
 */
#ifndef DITHERPIE_HIP_IDIFF_H
#define DITHERPIE_HIP_IDIFF_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_IDIFF_MAX_TAPS 12

/* The workspace dp_idiff_u8 needs for this call shape: the errors of the last two rows of a band of 64 rows, twice (the
 * band below reads one pair while the band after it writes the other), 32 * w bytes per frame.  0 for a negative n_frames
 * or an h or w < 1.  No HIP call. */
size_t dp_idiff_workspace_bytes(int64_t n_frames, int h, int w);

/* ---- Integer error diffusion ----
 *
 *   in_dev/out_dev  n_frames x h x w x 3 uint8, any address, distinct buffers (as for dp_error_diffusion_u8): out_dev ==
 *                   in_dev is refused, a partial overlap is not supported
 *   dx, dy, weight  n_taps int32 each, HOST memory, read during the call (the taps travel to the kernel by value)
 *   workspace_dev   dp_idiff_workspace_bytes(n_frames, h, w) bytes of device memory, 16-byte aligned, contents arbitrary:
 *                   the library writes what it reads from it
 * The nearest search is the table of ditherpie_hip_pattern.h, kept on the dp_palette, for a metric palette the one derived
 * from its top-2 table (ditherpie_hip_metric.h): the first dp_idiff_u8 / dp_dotdiff_u8 / dp_pattern_u8 with a palette builds
 * it on the caller's stream under the palette's build mutex; dp_pattern_prepare (dp_metric_prepare, then dp_pattern_prepare,
 * for a metric palette's two tables) builds it ahead of time.  Because the build allocates and synchronises, the FIRST call
 * with a palette must not happen while its stream is being captured into a graph.  With the table in place a call is
 * launches only: one workgroup per frame, one launch per 65535 frames.
 * n_frames == 0 (with valid arguments otherwise) returns DP_OK without a launch and touches nothing; in_dev, out_dev and
 * workspace_dev may then be NULL.
 * DP_EINVAL: a NULL pointer, n_frames < 0, h or w < 1, h * w > 2^30, a tap rule above broken, strength256 outside 0 .. 256,
 * out_dev == in_dev, a workspace that is not 16-byte aligned.  DP_EUNSUPPORTED: K > 256, a palette value outside [0, 255].
 * DP_EWORKSPACE: a workspace smaller than dp_idiff_workspace_bytes.
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_idiff_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, const dp_palette *pal,
                const int32_t *dx, const int32_t *dy, const int32_t *weight, int n_taps, int divisor, int strength256,
                void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_IDIFF_H */
