/*
 * ditherpie_hip_alpha.h -- transparency with libditherpie_hip.so: an RGBA source is split into the RGB the ditherer sees and a
 * one-byte mask of its transparent pixels, the two scan-free diffusions take that mask (a transparent pixel neither receives nor
 * hands on error, and its hidden colour is never looked at), and the results are put together again: a key index in an index plane
 * (PNG-8 with a tRNS chunk, 'P' images with info["transparency"]) or an RGBA frame.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument checks
 * before any HIP call, work enqueued asynchronously on the caller's stream, the calling thread's current device).
 * DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason ditherpie_hip_hold.h is: this header has
 * its own memory-discipline cases (tests/test_gpu_alpha_memory.py) and its own guard (tests/test_alpha_cpu.py).  Every device
 * entry point takes a descriptor whose first field is its own size, so its stream is a field and not a parameter: the
 * stalled-stream cases are in tests/test_gpu_alpha_streams.py.
 *
 * Definitions (tests/alpha_ref.py states them in numpy; csrc/host_logic.h: alpha_split, alpha_key, alpha_join).  All integer.
 *
 * Mask.  alpha is one byte per pixel, mask[y][x] is 1 (transparent) or 0 (opaque):
 *   DP_ALPHA_THRESHOLD   mask = alpha < threshold, threshold in 0 .. 256 (0: nothing is transparent, 256: everything is)
 *   DP_ALPHA_ORDERED     m in {2, 4, 8}, B_m the Bayer rank matrix (B_2 = [[0, 2], [3, 1]], B_2m = [[4B, 4B + 2], [4B + 3, 4B + 1]]):
 *                        mask = 2 m^2 alpha < 255 (2 B_m[(y0 + y) mod m][(x0 + x) mod m] + 1)
 *                        alpha 0 is always transparent and alpha 255 never is; over a full m x m tile of constant alpha a exactly
 *                        (2 m^2 a + 255) / 510 pixels (rounded down) are opaque.  (y0, x0) are the global coordinates of the
 *                        frame's first pixel, as in the ordered modes.
 * Matte.  The RGB handed to the ditherer does not depend on the mask: without a matte it is the source RGB, with a matte colour M
 *   it is (c alpha + M (255 - alpha) + 127) / 255 per channel, rounded down (alpha 255 gives c, alpha 0 gives M).
 * Key.   out_plane = mask ? key : plane, key in 0 .. 255 (one-byte planes).
 * Join.  rgba = mask ? (fill, 0) : (rgb, 255).
 * In key, join and the two diffusions any non-zero mask byte counts as transparent; dp_alpha_split_u8 writes 0 and 1.
 *
 * Masked integer error diffusion: the definition of ditherpie_hip_idiff.h with one addition.  At a pixel with mask != 0,
 *   out = fill and nothing else happens: its acc is never read, it has no error and no tap contributions.  Contributions that
 *   opaque pixels send to a masked pixel are lost.
 * Masked dot diffusion: the definition of ditherpie_hip_dotdiff.h with two changes.  A masked pixel writes fill and hands on
 *   nothing.  For an opaque pixel p, E is the set of neighbours inside the image, of greater class and NOT masked; W is summed over
 *   that E, so the error goes to the opaque neighbours instead of being lost, and a pixel whose E is empty drops it.
 *   Dependencies only shrink against the unmasked definition, so a matrix of reach <= DP_DOTDIFF_MAX_REACH is diffused exactly.
 * With an all-zero mask both are dp_idiff_u8 / dp_dotdiff_u8, byte for byte.
 */
#ifndef DITHERPIE_HIP_ALPHA_H
#define DITHERPIE_HIP_ALPHA_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_ALPHA_THRESHOLD 0
#define DP_ALPHA_ORDERED 1
#define DP_ALPHA_MAX_FRAMES 65535 /* frames per call of dp_alpha_split_u8, dp_alpha_key_u8 and dp_alpha_join_u8 */
#define DP_ALPHA_MAX_ORIGIN 1073741824 /* y0 and x0 lie in 0 .. 2^30 */

/* Every descriptor: struct_size is sizeof(the descriptor) of the caller (a later revision adds fields at the end and tells the
 * revisions apart by it); every buffer may sit at any address unless stated; stream is a hipStream_t (the _host_ twins ignore it).
 * Common refusals, DP_EINVAL: a NULL descriptor or a wrong struct_size; n_frames < 0; h or w < 1 or h * w >= 2^31; a NULL buffer
 * (n_frames > 0); an output that overlaps an input or another output.  DP_EUNSUPPORTED: n_frames > DP_ALPHA_MAX_FRAMES (split, key,
 * join).  n_frames == 0 (with valid arguments otherwise) returns DP_OK and touches nothing; the buffers may then be NULL.
 * A refused call launches nothing and names the function in dp_last_error(). */

/*   rgba_dev     n_frames x h x w x 4 uint8 (r, g, b, alpha)
 *   mode         DP_ALPHA_THRESHOLD or DP_ALPHA_ORDERED; threshold 0 .. 256 is read by the first, m (2, 4, 8), y0 and x0 (0 ..
 *                DP_ALPHA_MAX_ORIGIN) by the second -- the fields of the other mode are not looked at
 *   has_matte    0: rgb is the source RGB; otherwise it is composited over matte[3]
 *   rgb_dev      n_frames x h x w x 3 uint8
 *   mask_dev     n_frames x h x w uint8: 0 or 1
 *   masked_dev   n_frames int64, 8-byte aligned: the transparent pixels per frame (zeroed on the stream, then added to) */
typedef struct dp_alpha_split_args {
    size_t struct_size;
    const uint8_t *rgba_dev;
    int64_t n_frames;
    int h;
    int w;
    int mode;
    int threshold;
    int m;
    int y0;
    int x0;
    int has_matte;
    uint8_t matte[3];
    uint8_t *rgb_dev;
    uint8_t *mask_dev;
    int64_t *masked_dev;
    void *stream;
} dp_alpha_split_args;

/*   planes_dev   n_frames x h x w uint8 index planes
 *   mask_dev     n_frames x h x w uint8
 *   key          0 .. 255: what a masked pixel becomes
 *   out_dev      n_frames x h x w uint8; out_dev == planes_dev (in place) is allowed, any other overlap is refused */
typedef struct dp_alpha_key_args {
    size_t struct_size;
    const uint8_t *planes_dev;
    const uint8_t *mask_dev;
    int64_t n_frames;
    int h;
    int w;
    int key;
    uint8_t *out_dev;
    void *stream;
} dp_alpha_key_args;

/*   rgb_dev      n_frames x h x w x 3 uint8
 *   mask_dev     n_frames x h x w uint8
 *   fill         the colour bytes of a masked pixel (its alpha is 0)
 *   rgba_dev     n_frames x h x w x 4 uint8 */
typedef struct dp_alpha_join_args {
    size_t struct_size;
    const uint8_t *rgb_dev;
    const uint8_t *mask_dev;
    int64_t n_frames;
    int h;
    int w;
    uint8_t fill[3];
    uint8_t *rgba_dev;
    void *stream;
} dp_alpha_join_args;

/* The arguments of dp_idiff_u8 (ditherpie_hip_idiff.h: the same tap rules, the same dp_idiff_workspace_bytes, the same palette
 * rules, lut_in honoured, the same first-call table build) with mask_dev (n_frames x h x w uint8) and fill. */
typedef struct dp_alpha_idiff_args {
    size_t struct_size;
    const uint8_t *in_dev;
    const uint8_t *mask_dev;
    uint8_t *out_dev;
    int64_t n_frames;
    int h;
    int w;
    const dp_palette *pal;
    const int32_t *dx;
    const int32_t *dy;
    const int32_t *weight;
    int n_taps;
    int divisor;
    int strength256;
    uint8_t fill[3];
    void *workspace_dev;
    size_t workspace_bytes;
    void *stream;
} dp_alpha_idiff_args;

/* The arguments of dp_dotdiff_u8 (ditherpie_hip_dotdiff.h: the same matrix, reach and palette rules) with mask_dev and fill. */
typedef struct dp_alpha_dotdiff_args {
    size_t struct_size;
    const uint8_t *in_dev;
    const uint8_t *mask_dev;
    uint8_t *out_dev;
    int64_t n_frames;
    int h;
    int w;
    const dp_palette *pal;
    const uint8_t *classes_host;
    int m;
    int strength256;
    uint8_t fill[3];
    void *stream;
} dp_alpha_dotdiff_args;

/* ---- Split: RGBA -> RGB (through the matte), mask, masked pixels per frame ----
 * One clearing of masked_dev and ONE kernel launch on the stream; no allocation and no wait: legal in a graph capture.
 * DP_EINVAL beside the common ones: a mode that is neither; a threshold outside 0 .. 256 (DP_ALPHA_THRESHOLD); an m that is none of
 * 2, 4, 8 or a y0 or x0 outside 0 .. DP_ALPHA_MAX_ORIGIN (DP_ALPHA_ORDERED); a masked_dev that is not 8-byte aligned. */
int dp_alpha_split_u8(const dp_alpha_split_args *a);
/* The same on the CPU, every buffer in host memory: the host statement.  Needs no device; the same refusals. */
int dp_alpha_split_host_u8(const dp_alpha_split_args *a);

/* ---- Key: the key index at the masked pixels of index planes ----   One launch.  DP_EINVAL beside the common ones: a key outside
 * 0 .. 255. */
int dp_alpha_key_u8(const dp_alpha_key_args *a);
int dp_alpha_key_host_u8(const dp_alpha_key_args *a);

/* ---- Join: RGB and mask -> RGBA ----   One launch. */
int dp_alpha_join_u8(const dp_alpha_join_args *a);
int dp_alpha_join_host_u8(const dp_alpha_join_args *a);

/* ---- Masked integer error diffusion ----
 * As dp_idiff_u8: launches only once the palette's table is in place (the FIRST call with a palette builds it and must not
 * happen during a graph capture), one workgroup per frame, one launch per 65535 frames; h * w <= 2^30.  The refusals of
 * dp_idiff_u8, naming this function, and DP_EINVAL for a NULL mask_dev (n_frames > 0) and for an out_dev that overlaps in_dev or
 * mask_dev. */
int dp_alpha_idiff_u8(const dp_alpha_idiff_args *a);

/* ---- Masked dot diffusion ----
 * As dp_dotdiff_u8; its refusals, naming this function, and DP_EINVAL for a NULL mask_dev (n_frames > 0) and for an out_dev that
 * overlaps in_dev or mask_dev. */
int dp_alpha_dotdiff_u8(const dp_alpha_dotdiff_args *a);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_ALPHA_H */
