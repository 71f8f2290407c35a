/*
 * ditherpie_hip_clip.h -- clip-wide palettes with libditherpie_hip.so: the two device pieces a palette fitted to a whole
 * video needs beside dp_kmeans_hist_build_u8(accumulate = 1), dp_median_cut_host and the Lloyd passes over the histogram.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_indexed.h is one: the test suite pins the device entry points of ditherpie_hip.h to its memory-discipline
 * matrix; this header has its own matrix (tests/test_gpu_clip_memory.py) and its own guard (tests/test_clip_palette_cpu.py).
 */
#ifndef DITHERPIE_HIP_CLIP_H
#define DITHERPIE_HIP_CLIP_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Distinct colours in first-occurrence order over a STREAM of pixel buffers ----
 *
 * dp_distinct_first_u8 needs every pixel resident in one buffer; a clip (6 MB per 1080p frame) is not.  Here the caller
 * keeps, between calls, a STATE (the "seen" set: one bit per colour, dp_distinct_stream_state_bytes() = 2 MiB), the LIST
 * (3 * 2^24 bytes: every colour there is, so it cannot overflow) and its length (one int64 on the device).
 *
 * dp_distinct_stream_reset: clears the state and zeroes *n_distinct_dev (two memsets on `stream`).
 * dp_distinct_stream_add_u8: appends to list_dev, from entry *n_distinct_dev on, the colours of the n pixels of px_dev
 *   that no earlier add since the last reset has seen, in order of their first occurrence within px_dev; advances
 *   *n_distinct_dev and marks those colours seen.  After any sequence of adds the list and its length are those of
 *   dp_distinct_first_u8 over the concatenation of the buffers, byte for byte, however the stream was cut into buffers.
 *   Nothing is read back to the host.  n == 0 returns DP_OK without a launch and touches nothing.
 *
 * ORDERING: all calls that name one state (reset, add, and whatever reads the list or its length) are ordered on ONE
 * stream, or by the caller's events; two adds into one state must never run concurrently.
 *
 *   px_dev           n packed RGB pixels (3 * n bytes), any address; n < 2^32 - 16 per call
 *   state_dev        dp_distinct_stream_state_bytes() bytes, 16-byte aligned
 *   list_dev         3 * 2^24 bytes, any address
 *   n_distinct_dev   one int64, 8-byte aligned
 *   workspace_dev    dp_distinct_stream_workspace_bytes(n) bytes, 16-byte aligned: scratch of this call only (a 64 MB
 *                    first-index table + 1/8 byte per pixel), its contents before the call do not matter
 * DP_EINVAL: a NULL pointer (px_dev may be NULL when n == 0), n out of range, a misaligned state / counter, a workspace
 * that is NULL, misaligned or smaller than dp_distinct_stream_workspace_bytes(n).  A refused call launches nothing:
 * state, list and count are untouched. */
size_t dp_distinct_stream_state_bytes(void);
size_t dp_distinct_stream_workspace_bytes(int64_t n);
int dp_distinct_stream_reset(void *state_dev, int64_t *n_distinct_dev, void *stream);
int dp_distinct_stream_add_u8(const uint8_t *px_dev, int64_t n, void *state_dev, uint8_t *list_dev, int64_t *n_distinct_dev,
                              void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- Rank sample of a colour histogram ----
 *
 * hist_dev is a histogram of dp_kmeans_hist_build_u8 (dp_kmeans_hist_bytes() bytes).  Lay its pixels out in the
 * histogram's own slot order -- slot = (r>>4)<<20 | (g>>4)<<16 | (b>>4)<<12 | (r&15)<<8 | (g&15)<<4 | (b&15), every
 * colour repeated count times -- and out_dev[3 i ..] is the colour of the pixel with zero-based rank ranks_dev[i]: a
 * sample of the clip's colour MULTISET that does not depend on the order the pixels arrived in.  A rank < 0 or >= the
 * number of pixels writes (0, 0, 0) and ADDS one to *n_out_of_range_dev (the caller zeroes it).
 * One prefix sum over the histogram's 4096 per-cell totals, then per rank a binary search for its cell and a scan of that
 * cell's 16 KB slice (one wave per rank) -- never the 64 MB table.
 *
 *   ranks_dev            n_ranks int64, 8-byte aligned; 0 <= n_ranks <= 16384 (the sample limit of dp_kmeans_plusplus_u8)
 *   out_dev              3 * n_ranks bytes, any address
 *   n_out_of_range_dev   one int64, 8-byte aligned
 *   workspace_dev        dp_hist_sample_workspace_bytes() bytes, 16-byte aligned (the cell prefix sums)
 * DP_EINVAL: a NULL pointer, n_ranks out of range, hist_dev not 16-byte aligned, misaligned ranks / counter, a workspace
 * that is NULL, misaligned or too small.  n_ranks == 0 returns DP_OK without a launch. */
size_t dp_hist_sample_workspace_bytes(void);
int dp_hist_sample_u8(const void *hist_dev, const int64_t *ranks_dev, int n_ranks, uint8_t *out_dev, int64_t *n_out_of_range_dev,
                      void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_CLIP_H */
