/*
 * ditherpie_hip_resample.h -- filtered resize with libditherpie_hip.so: the BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS
 * filters of Pillow's Image.resize for packed RGB uint8 frames, bit-identical to Pillow, on frames that stay in device memory.
 * dp_resize_nearest_u8 (ditherpie_hip.h) stays what it is: one source pixel per output pixel.  This is the area / windowed-sinc
 * downscale that pixelization wants in front of the dither; it also enlarges.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument checks
 * before any HIP call, work enqueued asynchronously on the caller's stream, the calling thread's current device).
 * DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason ditherpie_hip_idiff.h is: the test suite
 * pins the device entry points of each header to a memory-discipline matrix; this header has its own
 * (tests/test_gpu_resample_memory.py) and its own guard (tests/test_resample_cpu.py).  dp_resample_u8 takes a descriptor, so its
 * stream is a field and not a parameter: its stalled-stream cases are in tests/test_gpu_resample_streams.py.
 *
 * Definition (tests/resample_ref.py states it in numpy; csrc/host_logic.h: resample_coeffs, resample_host).  Everything is
 * integer except the coefficients.
 *
 * Coefficients of one axis, for `in` source and `out` output positions and a filter (f, support) -- Pillow's precompute_coeffs
 * and normalize_coeffs_8bpc over the whole source extent.  float64, evaluated in exactly this order, no contraction:
 *   scale = in / out;  fs = max(scale, 1.0);  sup = support * fs;  ss = 1.0 / fs
 *   ksize = (int)ceil(sup) * 2 + 1
 *   for xx in 0 .. out-1:
 *       center = (xx + 0.5) * scale
 *       xmin = max((int)(center - sup + 0.5), 0)
 *       xmax = min((int)(center + sup + 0.5), in) - xmin            a count, not an end
 *       w[x] = f((x + xmin - center + 0.5) * ss)                    for x in 0 .. xmax-1
 *       ww = w[0] + w[1] + ... (left to right);  if ww != 0: w[x] /= ww
 *       k[x] = (int)(-0.5 + w[x] * 4194304) if w[x] < 0 else (int)(0.5 + w[x] * 4194304)      2^22, truncated toward zero
 * The filters:
 *   box       support 0.5:  1 if -0.5 < x <= 0.5, else 0
 *   bilinear  support 1:    x = |x|;  1 - x if x < 1, else 0
 *   hamming   support 1:    x = |x|;  1 at 0;  0 at x >= 1;  else x *= pi;  sin(x) / x * (0.54 + 0.46 * cos(x))
 *   bicubic   support 2, a = -0.5:  x = |x|;  ((a+2)*x - (a+3))*x*x + 1 if x < 1;  (((x-5)*x+8)*x-4)*a if x < 2;  else 0
 *   lanczos   support 3:    sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0;  sinc(0) = 1, otherwise x *= pi;  sin(x) / x
 * sin and cos are the C library's.
 *
 * One pass along an axis, for every output position and channel:
 *   out = clamp((2097152 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255)          an arithmetic shift: it floors negative sums
 *
 * A resize of h x w to oh x ow, in Pillow's order:
 *   the vertical coefficients first;  y0 = ymin[0],  y1 = ymin[oh-1] + ycount[oh-1]
 *   if ow != w: the horizontal pass over the source rows y0 .. y1-1 only, into a uint8 intermediate of (y1-y0) x ow x 3; the
 *               vertical bounds shift by -y0
 *   if oh != h: the vertical pass over that intermediate, or over the source when there was no horizontal pass
 *   equal sizes on an axis skip that pass; equal on both axes is a copy
 * Frames of a batch are independent.
 *
 * Limits: every size from 1 to 16384, h * w <= 2^30.  A plan in which 255 * sum |k| + 2^21 of some output position reaches 2^31
 * is refused (Pillow's int32 sum would overflow there too).
 */
#ifndef DITHERPIE_HIP_RESAMPLE_H
#define DITHERPIE_HIP_RESAMPLE_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_RESAMPLE_BOX 0
#define DP_RESAMPLE_BILINEAR 1
#define DP_RESAMPLE_HAMMING 2
#define DP_RESAMPLE_BICUBIC 3
#define DP_RESAMPLE_LANCZOS 4
#define DP_RESAMPLE_MAX_SIZE 16384

/* The coefficient tables of one resize geometry on one device. */
typedef struct dp_resample_plan dp_resample_plan;

/* Builds the coefficients of both axes on the host and uploads them (bounds and int32 k) to the calling thread's current device
 * with a blocking copy, as dp_thresholds_create uploads its table.  It takes no stream, allocates and waits: it is NOT legal while
 * a stream of the device is being captured into a graph -- make the plan first.
 * DP_EINVAL: a NULL `out`, a filter that is none of DP_RESAMPLE_*, a size outside 1 .. DP_RESAMPLE_MAX_SIZE, h * w > 2^30.
 * DP_EUNSUPPORTED: the int32 sum of a pass could overflow (see above). */
int dp_resample_plan_create(int filter, int h, int w, int oh, int ow, dp_resample_plan **out);
void dp_resample_plan_destroy(dp_resample_plan *plan);

/* The workspace dp_resample_u8 needs for n_frames frames: the intermediate, n_frames x (y1 - y0) x ow x 3 bytes rounded up to a
 * multiple of 16; 0 when one pass (or the copy) suffices, for a NULL plan and for n_frames < 1.  No HIP call. */
size_t dp_resample_workspace_bytes(const dp_resample_plan *plan, int64_t n_frames);

/* The arguments of dp_resample_u8.  struct_size is sizeof(dp_resample_args) of the caller: a later revision adds fields at the
 * end and tells the revisions apart by it.
 *   in_dev          n_frames x h x w x 3 uint8, any address
 *   out_dev         n_frames x oh x ow x 3 uint8, any address; a buffer distinct from in_dev (out_dev == in_dev is refused, a
 *                   partial overlap is not supported)
 *   plan            of the device the buffers live on
 *   workspace_dev   dp_resample_workspace_bytes(plan, n_frames) bytes of device memory, 16-byte aligned, contents arbitrary; may
 *                   be NULL when that is 0
 *   stream          a hipStream_t */
typedef struct dp_resample_args {
    size_t struct_size;
    const uint8_t *in_dev;
    uint8_t *out_dev;
    int64_t n_frames;
    const dp_resample_plan *plan;
    void *workspace_dev;
    size_t workspace_bytes;
    void *stream;
} dp_resample_args;

/* ---- Filtered resize ----
 * Launches only (one kernel per pass and 65535 frames; a copy on the stream when both sizes are equal): legal in a graph capture
 * from the first call.  n_frames == 0 (with valid arguments otherwise) returns DP_OK and touches nothing; in_dev, out_dev and
 * workspace_dev may then be NULL.
 * DP_EINVAL: a NULL descriptor, plan, in_dev or out_dev (or workspace_dev where a workspace is needed), a struct_size that is not
 * sizeof(dp_resample_args), n_frames < 0, out_dev == in_dev, a workspace that is not 16-byte aligned.
 * DP_EWORKSPACE: a workspace smaller than dp_resample_workspace_bytes.
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_resample_u8(const dp_resample_args *a);

/* The same resize on the CPU, host memory in and out: the host statement.  Needs no device.
 * DP_EINVAL / DP_EUNSUPPORTED as dp_resample_plan_create, and DP_EINVAL for a NULL pointer (with n > 0) or n < 0. */
int dp_resample_host(int filter, const uint8_t *in, uint8_t *out, int64_t n, int h, int w, int oh, int ow);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_RESAMPLE_H */
