/*
 * ditherpie_hip_hold.h -- temporal hold with libditherpie_hip.so: cells of a video whose SOURCE has not moved keep the palette
 * indices they already show, cells that changed take the fresh dither.  It sits between the dither (index planes of a batch of
 * frames) and the inter-frame delta / encoders (ditherpie_hip_gif.h, ditherpie_hip_png.h): a diffusion dither reorders everything
 * after one changed pixel and noise flips ordered pixels near a threshold, so without a hold consecutive planes are almost never
 * equal where nothing moves, and the delta finds nothing to drop.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument checks
 * before any HIP call, work enqueued asynchronously on the caller's stream, the calling thread's current device).
 * DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason ditherpie_hip_resample.h is: this header
 * has its own memory-discipline cases (tests/test_gpu_hold_memory.py) and its own guard (tests/test_hold_cpu.py).  dp_hold_u8
 * takes a descriptor, so its stream is a field and not a parameter: its stalled-stream cases are in tests/test_gpu_hold_streams.py.
 *
 * Definition (tests/hold_ref.py states it in numpy; csrc/host_logic.h: hold_apply).  Everything is integer.
 *   src      n_frames x h x w x 3 uint8: the frames as handed to the ditherer
 *   planes   n_frames x h x w uint8: their fresh dither as palette indices
 *   state    anchor h x w x 3 uint8 (the source of every pixel at its last refresh), held h x w uint8 (the index it shows),
 *            has_state (0: the first frame of a stream; the contents of anchor and held are then not read)
 *   cell in {1, 2, 4, 8, 16}, tol in 0 .. 255, share256 in 0 .. 256
 * The frame is cut into cell x cell cells from the top-left corner; the cells of the right and bottom edges are clipped, cell_px
 * is a cell's actual pixel count.  For f = 0 .. n_frames-1, in order:
 *   without state every pixel refreshes; otherwise
 *   a pixel p is CHANGED iff max over c of |src[f][p][c] - anchor[p][c]| > tol
 *   a cell REFRESHES iff changed_count > 0 and changed_count * 256 >= share256 * cell_px
 *   every pixel of a refreshing cell: anchor[p] = src[f][p], held[p] = planes[f][p]; the pixels of other cells keep both
 *   out[f] = held;  refreshed[f] = the number of pixels refreshed;  there is state from now on
 * After the call anchor and held are those of frame n_frames-1, so the result does not depend on how a stream is cut into calls.
 * The comparison is with the anchor, never with the frame before: slow drift accumulates and triggers a refresh.
 */
#ifndef DITHERPIE_HIP_HOLD_H
#define DITHERPIE_HIP_HOLD_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_HOLD_MAX_CELL 16
#define DP_HOLD_MAX_FRAMES 65535

/* The arguments of dp_hold_u8 and dp_hold_host_u8.  struct_size is sizeof(dp_hold_args) of the caller: a later revision adds
 * fields at the end and tells the revisions apart by it.  Every buffer may sit at any address, except refreshed_dev.
 *   src_dev         n_frames x h x w x 3 uint8
 *   planes_dev      n_frames x h x w uint8
 *   anchor_dev      h x w x 3 uint8, read (with has_state) and written
 *   held_dev        h x w uint8, read (with has_state) and written
 *   has_state       0: anchor_dev and held_dev are written only
 *   out_dev         n_frames x h x w uint8; it overlaps none of the other buffers
 *   refreshed_dev   n_frames int64, 8-byte aligned; written by the call (zeroed on the stream, then added to)
 *   stream          a hipStream_t (dp_hold_host_u8 ignores it) */
typedef struct dp_hold_args {
    size_t struct_size;
    const uint8_t *src_dev;
    const uint8_t *planes_dev;
    int64_t n_frames;
    int h;
    int w;
    int cell;
    int tol;
    int share256;
    uint8_t *anchor_dev;
    uint8_t *held_dev;
    int has_state;
    uint8_t *out_dev;
    int64_t *refreshed_dev;
    void *stream;
} dp_hold_args;

/* ---- Temporal hold ----
 * One clearing of refreshed_dev and ONE kernel launch on the stream, whatever n_frames (the loop over the frames is inside the
 * kernel); no allocation and no wait: legal in a graph capture.  n_frames == 0 (with valid arguments otherwise) returns DP_OK and
 * touches nothing; the buffers may then be NULL.
 * DP_EINVAL: a NULL descriptor or a struct_size that is not sizeof(dp_hold_args); n_frames < 0; a NULL buffer (n_frames > 0); h or
 * w < 1 or h * w >= 2^31; a cell that is none of 1, 2, 4, 8, 16; tol outside 0 .. 255; share256 outside 0 .. 256; a refreshed_dev
 * that is not 8-byte aligned; out_dev overlapping planes_dev, src_dev, anchor_dev, held_dev or refreshed_dev; the state (anchor_dev,
 * held_dev) or refreshed_dev overlapping the inputs or each other.
 * DP_EUNSUPPORTED: n_frames > DP_HOLD_MAX_FRAMES.
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_hold_u8(const dp_hold_args *a);

/* The same on the CPU, every buffer in host memory: the host statement.  Needs no device; the same refusals. */
int dp_hold_host_u8(const dp_hold_args *a);

/* The sizes of the two state buffers of an h x w stream: *anchor_bytes = 3 h w, *held_bytes = h w.  No HIP call.
 * DP_EINVAL: a NULL pointer, h or w < 1 or h * w >= 2^31. */
int dp_hold_state_bytes(int h, int w, size_t *anchor_bytes, size_t *held_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_HOLD_H */
