/*
 * ditherpie_hip_png.h -- PNG-8 output with libditherpie_hip.so: the zlib stream (the contents of the IDAT chunks) of planes
 * of palette indices, compressed while the planes are resident in HBM.  The container around it (signature, IHDR, PLTE, IDAT
 * framing, chunk CRCs, IEND) is written by the caller (dither_pie_amd/png.py).
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_gif.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_png_memory.py) and its own guard (tests/test_png_cpu.py).
 */
#ifndef DITHERPIE_HIP_PNG_H
#define DITHERPIE_HIP_PNG_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The stream ----
 *
 * The host statement dp_png_deflate_host_u8 is normative; the device writes the same bytes for every input.
 *
 * Filtered bytes of a plane of h x w one-byte indices at bit depth d in {1, 2, 4, 8}: each row is a filter byte 0 and
 * ceil(w * d / 8) packed bytes, the leftmost pixel in the high-order bits, unused low bits of a row's last byte zero.
 * F = h * (1 + ceil(w * d / 8)) of them.  They exist only inside the encoder.  An index >= 1 << d is the caller's error; it
 * is encoded as index & ((1 << d) - 1) and never reaches an address computation.
 *
 * Per frame a complete zlib stream: 78 01, deflate blocks, the Adler-32 of the filtered bytes big-endian.
 *   - The filtered bytes are cut into segments of seg_bytes (the last may be shorter; a seg_bytes beyond F is one segment).
 *     Segments are compressed independently: no match reaches before its own segment's first byte.
 *   - One data block per segment, starting on a byte boundary.  Every segment but the last is followed by an empty stored
 *     block (three zero bits, padding to a byte, 00 00 FF FF); the data block of the last segment carries BFINAL.
 *   - Matches: minimum 3, maximum 258.  The one candidate of position p (p + 2 < n, n the segment's length) is the largest
 *     q < p in the segment whose three bytes hash alike: ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1 mod 2^32) >> 20.  Its
 *     length is the number of equal bytes up to min(258, n - p).  Greedy: a candidate of length >= 3 is always taken.
 *   - The block type is the smallest of stored and fixed-Huffman in bytes of the whole segment, the realigning block
 *     included; a tie goes to stored.  These entry points write no dynamic-Huffman blocks: the entry points of
 *     ditherpie_hip_png_dyn.h add them as a third candidate, with a larger workspace, and leave these bytes as they are.
 * Segments are what the device compresses independently (one wave each): a smaller seg_bytes costs file size (a cold
 * matcher and up to 5 bytes of realignment per segment) and buys parallelism.  A decoder sees an ordinary stream.
 *
 * dp_png_filtered_bytes: F.  dp_png_deflate_bound_bytes: the size no frame exceeds, 2 + F + 10 * n_seg + 4 with
 * n_seg = ceil(F / min(seg_bytes, F)): every segment stored (5 bytes of block header) and realigned (5 bytes).  Both are 0
 * for arguments the encoder refuses.
 *
 *   planes_dev   n_frames planes of h * w bytes back to back, any address
 *   out_dev      frame f's bytes start at out_dev + f * out_stride, any address; bytes past sizes_dev[f] within the stride
 *                are unspecified, no byte outside [out_dev, out_dev + n_frames * out_stride) is written
 *   sizes_dev    n_frames int64, 8-byte aligned: the byte count of each frame's stream
 *   ws_dev       dp_png_deflate_workspace_bytes(n_frames, h, w, depth, seg_bytes) bytes, 16-byte aligned; what it held does
 *                not matter
 * DP_EINVAL: a NULL pointer, h or w < 1, a depth outside {1, 2, 4, 8}, seg_bytes outside 256 ... 32768, F >= 2^31,
 * n_frames < 0, out_stride < dp_png_deflate_bound_bytes(h, w, depth, seg_bytes), a misaligned sizes_dev or ws_dev.
 * DP_EWORKSPACE: ws_bytes too small.  DP_EUNSUPPORTED: n_frames > 65535, or n_frames * n_seg >= 2^31 (cut the batch).
 * n_frames == 0 returns DP_OK without a launch and touches nothing.  A refused call launches nothing. */
size_t dp_png_filtered_bytes(int h, int w, int depth);
size_t dp_png_deflate_bound_bytes(int h, int w, int depth, int seg_bytes);
size_t dp_png_deflate_workspace_bytes(int n_frames, int h, int w, int depth, int seg_bytes);
int dp_png_deflate_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_dev,
                             int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* The same bytes computed on the host (host_logic.h: png_deflate_encode), no device involved: planes, out and sizes are host
 * memory.  The statement the device encoder is tested against, and what a container writer can run on without a GPU.
 * DP_EINVAL as above (without the alignment and workspace rules); n_frames == 0 returns DP_OK. */
int dp_png_deflate_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_host,
                           int64_t out_stride, int64_t *sizes_host);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_PNG_H */
