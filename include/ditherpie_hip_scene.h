/*
 * ditherpie_hip_scene.h -- scene-cut detection with libditherpie_hip.so: a coarse colour signature per frame and the
 * distance between the signatures of consecutive frames, computed while the frames are resident in HBM.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_indexed.h and ditherpie_hip_clip.h are: the test suite pins the device entry points of each header to a
 * memory-discipline matrix; this header has its own (tests/test_gpu_scene_memory.py) and its own guard
 * (tests/test_scenes_cpu.py).
 */
#ifndef DITHERPIE_HIP_SCENE_H
#define DITHERPIE_HIP_SCENE_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_SCENE_BINS 4096 /* 16 x 16 x 16 cells of the colour cube */

/* ---- Frame signatures ----
 *
 * sig_dev[f * 4096 + bin] = the number of pixels of frame f whose colour lies in the cell
 * bin = (r >> 4) << 8 | (g >> 4) << 4 | (b >> 4) -- the cell id of the colour histogram (slot >> 12 in
 * ditherpie_hip_clip.h).  Every row sums to h * w.  Integer counts: exact, and the same on every run.
 * The call zeroes sig_dev on `stream` itself (what the buffer held before does not matter), then ONE launch serves the
 * whole batch.
 *
 *   frames_dev   n_frames packed RGB frames of h x w pixels back to back (3 * h * w * n_frames bytes), any address
 *   sig_dev      n_frames * 4096 uint32, 16-byte aligned
 * DP_EINVAL: a NULL pointer, h or w < 1, n_frames < 0, h * w >= 2^32, sig_dev not 16-byte aligned.
 * DP_EUNSUPPORTED: n_frames > 65535 (cut the batch).  n_frames == 0 returns DP_OK without a launch and touches nothing.
 * A refused call launches nothing. */
int dp_frame_signatures_u8(const uint8_t *frames_dev, int n_frames, int h, int w, uint32_t *sig_dev, void *stream);

/* ---- Distances of consecutive signatures ----
 *
 * dist_dev[i] = sum over the 4096 bins of |sig[i][bin] - sig[i-1][bin]| for 1 <= i < n_frames; dist_dev[0] is the same
 * against prev_sig_dev when has_prev is non-zero, and 0 otherwise.  0 for frames with the same signature, 2 * h * w for
 * frames that share no cell.  After the distances sig[n_frames - 1] is copied into prev_sig_dev (on `stream`, behind the
 * reads), so that the next batch of the same stream of frames continues where this one ended: the caller keeps
 * prev_sig_dev between calls and passes has_prev = 0 for the first batch (and after a cut it wants to forget).
 *
 *   sig_dev        n_frames * 4096 uint32, 16-byte aligned
 *   prev_sig_dev   4096 uint32, 16-byte aligned; read only when has_prev is non-zero, always written (n_frames > 0)
 *   dist_dev       n_frames int64, 8-byte aligned
 * DP_EINVAL: a NULL pointer, n_frames < 0, a misaligned buffer.  n_frames == 0 returns DP_OK without a launch and leaves
 * prev_sig_dev as it is.  A refused call launches nothing. */
int dp_signature_distances(const uint32_t *sig_dev, int n_frames, uint32_t *prev_sig_dev, int has_prev, int64_t *dist_dev,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_SCENE_H */
