/*
 * ditherpie_hip_metric.h -- a perceptual colour metric for libditherpie_hip.so: palettes whose "nearest" is measured in an
 * integer Oklab instead of RGB, an exact table of the two nearest entries of every colour built on the device, and ordered
 * dithering that is one gather from that table per pixel.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_pattern.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_metric_memory.py) and its own guard (tests/test_metric_cpu.py).
 *
 * Definition (all integer arithmetic, >> floors; tests/metric_ref.py states it in numpy).
 *   LIN[v]  = round(65535 f(v / 255)), v = 0 .. 255; f(u) = u / 12.92 for u <= 0.04045, else ((u + 0.055) / 1.055)^2.4
 *             (a literal table in the library; LIN[1, 10, 11, 12, 128, 254] = 20, 199, 219, 241, 14146, 64952)
 *   (l,m,s) = (A . (LIN[r], LIN[g], LIN[b])) >> 16,  A = [[27015, 35149, 3372], [13887, 44611, 7038], [5787, 18463, 41286]]
 *             (each row sums to 65536; unsigned 32-bit products)
 *   c       = floor(cbrt(x * 2^32)) per component: the exact integer cube root, 0 .. 65535
 *   (L,a,b) = (B . (cl, cm, cs)) >> 14,  B = [[862, 3251, -17], [8102, -9948, 1846], [106, 3206, -3312]]   (signed 32-bit sums)
 *             (row sums 4096, 0, 0: greys have a = b = 0 exactly, white is (16383, 0, 0))
 *   d(q, k) = dL^2 + da^2 + db^2                          (at most 408 098 306 over the whole cube: int32)
 *   nearest, second = the two smallest (d(q, k), k), compared as pairs: the LOWEST INDEX wins on equal distance (not scipy's
 *             order: the metric is this library's to define).  K = 1: second = nearest = 0.
 *   ordered decision with the matrix value t (float32) at ((y0 + y) mod th_h, (x0 + x) mod th_w):
 *             f = double(d0) / (double(d0) + double(d1)), f = 0 when the sum is 0; the pixel takes nearest iff f <= double(t),
 *             else second; the output bytes are out_colors[index].
 *
 * What a metric palette means to the rest of the library: dp_pattern_u8, dp_pattern_prepare, dp_dotdiff_u8 and dp_idiff_u8
 * (ditherpie_hip_idiff.h: the scan error diffusion that takes a metric palette) use the metric
 * (their definitions stay as they are, only nearest(q) changes; their rank table is derived from the table below, 16 MiB
 * more); dp_palette_build_accel returns DP_OK and builds nothing; every other entry point that searches a palette
 * (dp_ordered_u8, dp_error_diffusion_u8, dp_error_diffusion_numba_u8, dp_hybrid_numba_u8, dp_riemersma_u8, dp_halftone_u8,
 * dp_wavelet_u8, dp_variable_diffusion_u8, dp_variance_gate_u8, dp_cells_u8) refuses it with DP_EUNSUPPORTED, names itself in
 * dp_last_error() and launches nothing: none of them falls back to RGB.
 */
#ifndef DITHERPIE_HIP_METRIC_H
#define DITHERPIE_HIP_METRIC_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_METRIC_RGB 0
#define DP_METRIC_OKLAB 1
#define DP_METRIC_TABLE_BYTES 33554432 /* two bytes per colour of the 2^24 cube: nearest | second << 8 */

/* dp_palette_create with a metric, fixed at birth, and without lut_in.  DP_METRIC_RGB gives a palette identical to
 * dp_palette_create(pal_f32, out_colors, K, NULL, out).  DP_METRIC_OKLAB needs K <= 256 and integer palette values in
 * [0, 255]: otherwise DP_EUNSUPPORTED.  DP_EINVAL: an unknown metric, and what dp_palette_create refuses.
 * dp_palette_metric: the metric of a palette (-1 for NULL); no HIP call. */
int dp_palette_create_metric(const float *pal_f32, const uint8_t *out_colors, int K, int metric, dp_palette **out);
int dp_palette_metric(const dp_palette *pal);

/* ---- The top-2 table ----
 *
 * nearest | second << 8 of all 2^24 colours, two bytes per colour in the 4 x 4 x 4 brick order of the pattern table, built by
 * one brute-force kernel (no pruning, no tree: the pair comparison gives exact ties by construction; K = 1 is a memset).  It
 * is kept on the dp_palette (32 MiB plus 5 KiB of records, freed by dp_palette_destroy) and is built once, lazily, under the
 * palette's build mutex: dp_metric_prepare builds it on the null stream, the first dp_metric_ordered_u8 / dp_pattern_u8 /
 * dp_dotdiff_u8 with the palette builds it on the caller's stream; either waits for the build before it publishes the table to
 * other threads.  Because the build allocates and synchronises, the FIRST such call with a palette must not happen while its
 * stream is being captured into a graph: call dp_metric_prepare before the capture.  Synchronous and idempotent; a failed
 * build leaves no table and the next call retries.
 * DP_EINVAL: a NULL palette, a palette of DP_METRIC_RGB.
 * dp_metric_table_bytes: the device memory the table of this palette takes once built (0 for a NULL palette or one of
 * DP_METRIC_RGB); no HIP call. */
int dp_metric_prepare(dp_palette *pal);
size_t dp_metric_table_bytes(const dp_palette *pal);

/* ---- Ordered dithering under the metric ----
 *
 *   in_dev/out_dev  n_frames x h x w x 3 uint8, any address; out_dev may be in_dev itself (a lane reads its pixels before
 *                   it writes them), a partial overlap is not supported
 *   (y0, x0)        global coordinates of pixel (0,0) of every frame (row-band / tile sharding)
 *   mode            DP_MODE_NEAREST: the nearest entry (thr may be NULL).  DP_MODE_MATRIX: the ordered decision above with
 *                   the float32 values of thr, any size.  DP_MODE_IGN: DP_EUNSUPPORTED.
 * One launch per 65535 frames.  n_frames == 0 (with a palette and valid sizes) returns DP_OK without a launch and touches
 * nothing, pointers may then be NULL.
 * DP_EINVAL: a NULL pointer, n_frames < 0, h or w < 1, h * w > 2^30, negative y0 or x0, y0 + h or x0 + w > 2^30, an unknown
 * mode, DP_MODE_MATRIX without thr, a palette of DP_METRIC_RGB.  A refused call launches nothing and names the function in
 * dp_last_error(). */
int dp_metric_ordered_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int h, int w, int y0, int x0,
                         const dp_palette *pal, int mode, const dp_thresholds *thr, void *stream);

/* (L, a, b) of n_px packed RGB pixels (any address) as 3 x int32 per pixel (lab_dev 4-byte aligned), by the device function
 * the kernels above use.  n_px == 0 is a no-op.  DP_EINVAL: a NULL pointer, n_px < 0 or > 2^31 - 1, a misaligned lab_dev. */
int dp_metric_lab_u8(const uint8_t *in_dev, int32_t *lab_dev, int64_t n_px, void *stream);

/* ---- The host statements (pure host code: no HIP call, no device) ----
 *
 * dp_metric_lab_host: lab_host receives n x 3 int32.  DP_EINVAL: a NULL pointer, n < 0.
 * dp_metric_top2_host: idx0 / idx1 receive nearest / second of n packed RGB colours for the palette pal_f32 [K, 3] under
 * `metric` (DP_METRIC_RGB: squared Euclidean distance of the bytes, under the same pair order).  DP_EINVAL: a NULL pointer,
 * n < 0, K < 1, an unknown metric.  DP_EUNSUPPORTED: K > 256, a palette value that is no integer in [0, 255]. */
int dp_metric_lab_host(const uint8_t *rgb_host, int64_t n, int32_t *lab_host);
int dp_metric_top2_host(const uint8_t *rgb_host, int64_t n, const float *pal_f32, int K, int metric, uint8_t *idx0_host,
                        uint8_t *idx1_host);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_METRIC_H */
