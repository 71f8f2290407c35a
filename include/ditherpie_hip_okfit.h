/*
 * ditherpie_hip_okfit.h -- palettes fitted in the integer Oklab of ditherpie_hip_metric.h with libditherpie_hip.so: a weighted
 * k-means over the distinct colours of a colour histogram that is all integer, free of addition order and exact.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, the calling thread's current device).  DP_ABI_VERSION is
 * unchanged: these are additions.  A header of its own for the reason ditherpie_hip_metric.h is: the test suite pins the device
 * entry points of each header to a memory-discipline matrix; this header has its own (tests/test_gpu_okfit_memory.py) and its
 * own guard (tests/test_okfit_cpu.py).
 *
 * Definition (all integer arithmetic, divisions floor; tests/okfit_ref.py states it in numpy).
 *   points    the n distinct colours of the input in ascending order of code = r << 16 | g << 8 | b; count[i] >= 1, the sum of
 *             the counts below 2^32 (the caller's contract; a histogram guarantees it); P[i] = (L, a, b) of colour i
 *   d         dL^2 + da^2 + db^2, at most 408 098 306; centres are means of points, the bound holds for them too
 *   seeding   centre 0 = P of the point with the largest count, the lowest code on ties; for j = 1 .. K - 1, with dmin[i] the
 *             distance of point i to the nearest centre chosen so far, centre j = P of the point that maximises the 64-bit
 *             product count[i] * dmin[i], the lowest code on ties; if that maximum is 0 centre j repeats centre 0
 *   Lloyd     at most max_iter times: (1) every point takes the centre of least d, the lowest centre index on ties; (2) a
 *             centre with members becomes (2 S + cnt) / (2 cnt) per component, cnt = sum count, S = sum count * P in int64
 *             (half rounds up, the division floors for negatives), a centre without members keeps its value; (3) stop when no
 *             centre changed.  n_iter counts the assignment passes of this loop.
 *   bytes     one more assignment against the final centres; palette entry k is the colour of the member of k that is nearest
 *             to centre k, the lowest code on ties; a centre without members searches all points.  Entries are in the order of
 *             the centres; duplicates are possible when n < K and are kept.
 *   results   the palette, K x 3 uint8; the final centres, K x 3 int32; n_iter; the distortion sum count * d(point, its centre)
 *             of that last assignment, uint64
 * A pure function of the colour multiset: no random numbers, no dependence on pixel order, batching or frame order.
 */
#ifndef DITHERPIE_HIP_OKFIT_H
#define DITHERPIE_HIP_OKFIT_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_OKFIT_MAX_COLORS 256
#define DP_OKFIT_MAX_ITER 10000
#define DP_OKFIT_MAX_POINTS 16777216 /* every colour there is */
#define DP_OKFIT_POINT_BYTES 16      /* a point record: uint32 code, uint32 count, int16 L, a, b, int16 zero */

/* ---- Points from a colour histogram ----
 *
 * hist_dev is a histogram of dp_kmeans_hist_build_u8 (dp_kmeans_hist_bytes() bytes, 16-byte aligned; it is only read).
 * dp_okfit_hist_count: *n_dev receives the number of colours with a count above zero.
 * dp_okfit_hist_points: *n_dev receives that number too, and points_dev the records of the first min(n, capacity) occupied
 *   colours in ascending code order.  When n exceeds the capacity the true n is still reported, nothing past the capacity is
 *   written and the call returns DP_OK: the caller compares.  capacity == 0 writes no record (points_dev may then be NULL).
 * Both are asynchronous on `stream`; nothing is read back to the host.
 *
 *   n_dev            one int64, 8-byte aligned
 *   points_dev       capacity records of DP_OKFIT_POINT_BYTES, 16-byte aligned; 0 <= capacity <= DP_OKFIT_MAX_POINTS
 *   workspace_dev    dp_okfit_hist_workspace_bytes() bytes, 16-byte aligned: scratch of this call only, its contents before
 *                    the call do not matter
 * DP_EINVAL: a NULL pointer, a misaligned hist_dev / points_dev / n_dev, a capacity out of range, a workspace that is NULL,
 * misaligned or too small.  A refused call launches nothing. */
size_t dp_okfit_hist_workspace_bytes(void);
int dp_okfit_hist_count(const void *hist_dev, int64_t *n_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int dp_okfit_hist_points(const void *hist_dev, void *points_dev, int64_t capacity, int64_t *n_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);

/* ---- Points from arrays ----
 *
 * points_dev receives the records of n colours given as codes_dev[i] = r << 16 | g << 8 | b and counts_dev[i] (uint32 each,
 * 4-byte aligned).  The caller's contract, which the device cannot refuse: codes strictly ascending and below 2^24, counts >= 1,
 * their sum below 2^32.  Asynchronous.  n == 0 returns DP_OK without a launch.
 * DP_EINVAL: a NULL pointer, n < 0 or > DP_OKFIT_MAX_POINTS, misaligned codes_dev / counts_dev (4) or points_dev (16). */
int dp_okfit_points_u32(const uint32_t *codes_dev, const uint32_t *counts_dev, int64_t n, void *points_dev, void *stream);

/* ---- The fit ----
 *
 *   points_dev       n records as the calls above write them (16-byte aligned; only read)
 *   palette_dev      3 * K bytes, any address
 *   centres_dev      3 * K int32, 4-byte aligned
 *   distortion_dev   one uint64, 8-byte aligned
 *   n_iter_out       one int in HOST memory
 *   workspace_dev    dp_okfit_workspace_bytes(n, K) bytes, 16-byte aligned: scratch of this call only (the working centres, the
 *                    int64 totals, 4 bytes of dmin per point), its contents before the call do not matter
 * The seeding, every Lloyd pass, the centre update and the medoid search run on the device; no centre travels through the host.
 * After each update the host reads ONE word (did a centre change?) to decide whether to go on, so the call synchronises
 * `stream` once per pass and returns with every result written: it must not be made while the stream is captured into a graph.
 * DP_EINVAL: a NULL pointer, n < 1 or > DP_OKFIT_MAX_POINTS, K < 1, max_iter < 1 or > DP_OKFIT_MAX_ITER, a misaligned pointer,
 * a workspace that is NULL, misaligned or smaller than dp_okfit_workspace_bytes(n, K).  DP_EUNSUPPORTED: K >
 * DP_OKFIT_MAX_COLORS.  A refused call launches nothing and names the function in dp_last_error().
 * dp_okfit_workspace_bytes: 0 for arguments the fit refuses. */
size_t dp_okfit_workspace_bytes(int64_t n, int K);
int dp_okfit_fit(const void *points_dev, int64_t n, int K, int max_iter, uint8_t *palette_dev, int32_t *centres_dev,
                 uint64_t *distortion_dev, int *n_iter_out, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- The host statement (pure host code: no HIP call, no device) ----
 *
 * The definition above on host arrays: codes / counts n uint32 each, palette K x 3 uint8, centres K x 3 int32.
 * DP_EINVAL: a NULL pointer, n < 1 or > DP_OKFIT_MAX_POINTS, K < 1, max_iter out of range, codes that are not strictly
 * ascending or not below 2^24, a count of 0, counts whose sum is 2^32 or more.  DP_EUNSUPPORTED: K > DP_OKFIT_MAX_COLORS. */
int dp_okfit_host(const uint32_t *codes, const uint32_t *counts, int64_t n, int K, int max_iter, uint8_t *palette, int32_t *centres,
                  int *n_iter_out, uint64_t *distortion_out);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_OKFIT_H */
