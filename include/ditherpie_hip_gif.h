/*
 * ditherpie_hip_gif.h -- animated GIF output with libditherpie_hip.so: inter-frame deltas of one-byte index planes and the
 * LZW image data of every frame, computed while the planes are resident in HBM.  The container around them (header, colour
 * tables, control blocks) is a few bytes per frame and is written by the caller (dither_pie_amd/gif.py).
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_scene.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_gif_memory.py) and its own guard (tests/test_gif_cpu.py).
 */
#ifndef DITHERPIE_HIP_GIF_H
#define DITHERPIE_HIP_GIF_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Inter-frame deltas ----
 *
 * out[f][p] = transparent where planes[f][p] == planes[f-1][p], else planes[f][p], for 1 <= f < n_frames; frame 0 is
 * compared with prev_plane_dev when has_prev is non-zero and copied through otherwise.  The comparison is always with the
 * ORIGINAL plane before, never with a delta.  changed_dev[f] = the number of pixels of frame f that differ from the plane
 * before (n_px for a frame 0 without one): 0 marks a frame that repeats its predecessor.  After the reads
 * planes[n_frames - 1] is copied into prev_plane_dev (on `stream`), so that the next batch of the same stream of frames
 * continues where this one ended: the caller keeps prev_plane_dev between calls and passes has_prev = 0 for the first batch.
 *
 *   planes_dev       n_frames planes of n_px bytes back to back, any address
 *   prev_plane_dev   n_px bytes, any address; read only when has_prev is non-zero, always written (n_frames > 0)
 *   out_dev          n_frames * n_px bytes, any address; must not overlap planes_dev or prev_plane_dev
 *   changed_dev      n_frames int64, 8-byte aligned; zeroed by the call itself
 * DP_EINVAL: a NULL pointer, n_px < 1, n_frames < 0, transparent outside 0 ... 255, changed_dev misaligned, out_dev inside
 * the planes or the carried plane (or the reverse: in-place operation is refused), prev_plane_dev inside the planes.
 * DP_EUNSUPPORTED: n_frames > 65535 (cut the batch).  n_frames == 0 returns DP_OK without a launch and touches nothing.
 * A refused call launches nothing. */
int dp_index_delta_u8(const uint8_t *planes_dev, int n_frames, int64_t n_px, uint8_t *prev_plane_dev, int has_prev, int transparent,
                      uint8_t *out_dev, int64_t *changed_dev, void *stream);

/* ---- LZW image data ----
 *
 * For each frame: the min_code_size byte, the code stream in sub-blocks of at most 255 bytes each behind its length byte,
 * and the zero terminator -- what a GIF file holds between an image descriptor (or local colour table) and the next block.
 *
 * The stream (the host statement dp_gif_lzw_host_u8 is normative; the device writes the same bytes for every input):
 *   - Clear = 1 << min_code_size, EOI = Clear + 1, the first free code is Clear + 2, codes are packed LSB first.
 *   - The h * w pixels in raster order are cut into chunks of chunk_px (the last may be shorter; a chunk_px beyond h * w is
 *     the whole frame).  Every chunk opens with a Clear, written at the width in force at the end of the chunk before; the
 *     first of a frame at min_code_size + 1.  Behind a Clear the width is min_code_size + 1 and the dictionary is empty.
 *   - Within a chunk: greedy longest match.  After a code is emitted the pair (code, next pixel) gets the next free code
 *     while that is < 4096; the width grows by one when the entry just added is numbered 1 << width and the width is < 12.
 *     When no code is free, the emitted code is followed by a Clear at 12 bits and the dictionary starts over.
 *   - After the LAST code of a chunk no entry is added, but the width advances as if one had been (a decoder adds its
 *     lagging entry on reading that code).  When no code is free at that point nothing follows the code: the width stays
 *     12 and the next chunk's Clear (or EOI) is written at 12 bits.
 *   - EOI follows the last chunk at the width then in force.
 *   - A pixel >= 1 << min_code_size is the caller's error; it is encoded as pixel & ((1 << min_code_size) - 1).  No such
 *     value reaches an address computation.
 * Chunks are what the device compresses independently (one wave each); a smaller chunk_px costs file size (a Clear and a
 * cold dictionary per chunk) and buys parallelism.  A decoder sees an ordinary stream.
 *
 * dp_gif_lzw_bound_bytes: the size no frame exceeds.  Every code but a Clear and EOI consumes at least one pixel, so a
 * frame has at most n_px such codes; a Clear inside a chunk follows at least 4096 - 258 = 3838 codes that added an entry
 * and the one that found none free, so there are at most n_px / 3839 of them; n_chunks = ceil(n_px / min(chunk_px, n_px))
 * leading Clears; one EOI.  At 12 bits each that is D = ceil(12 * (n_px + n_px / 3839 + n_chunks + 1) / 8) data bytes,
 * and the frame is 1 + D + ceil(D / 255) + 1 bytes.  0 for arguments the encoder refuses.
 *
 *   planes_dev   n_frames planes of h * w bytes back to back, any address
 *   out_dev      frame f's bytes start at out_dev + f * out_stride, any address; bytes past sizes_dev[f] within the stride
 *                are unspecified, no byte outside [out_dev, out_dev + n_frames * out_stride) is written
 *   sizes_dev    n_frames int64, 8-byte aligned: the byte count of each frame
 *   ws_dev       dp_gif_lzw_workspace_bytes(n_frames, h, w, chunk_px) bytes, 16-byte aligned; what it held does not matter
 * DP_EINVAL: a NULL pointer, h or w < 1, h * w >= 2^31, n_frames < 0, min_code_size outside 2 ... 8, chunk_px < 1,
 * out_stride < dp_gif_lzw_bound_bytes(h, w, chunk_px), a misaligned sizes_dev or ws_dev.  DP_EWORKSPACE: ws_bytes too small.
 * DP_EUNSUPPORTED: n_frames > 65535, or n_frames * n_chunks >= 2^31 (cut the batch).  n_frames == 0 returns DP_OK without
 * a launch and touches nothing.  A refused call launches nothing. */
size_t dp_gif_lzw_bound_bytes(int h, int w, int64_t chunk_px);
size_t dp_gif_lzw_workspace_bytes(int n_frames, int h, int w, int64_t chunk_px);
int dp_gif_lzw_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int min_code_size, int64_t chunk_px, uint8_t *out_dev,
                         int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* The same bytes computed on the host (host_logic.h: gif_lzw_encode), no device involved: planes, out and sizes are host
 * memory.  The statement the device encoder is tested against, and what a container writer can run on without a GPU.
 * DP_EINVAL as above (without the alignment and workspace rules); n_frames == 0 returns DP_OK. */
int dp_gif_lzw_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int min_code_size, int64_t chunk_px, uint8_t *out_host,
                       int64_t out_stride, int64_t *sizes_host);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_GIF_H */
