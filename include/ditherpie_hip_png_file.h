/*
 * ditherpie_hip_png_file.h -- finished PNG chunks with libditherpie_hip.so: the CRC-32 of byte runs that are resident in HBM,
 * and the IDAT / fdAT chunks around the zlib streams of ditherpie_hip_png.h, packed back to back on the device.  What is left
 * to the caller (dither_pie_amd/png.py, dither_pie_amd/apng.py) is the bytes that do not depend on the pixels -- signature,
 * IHDR, PLTE, tRNS, acTL, fcTL, IEND --, which it hands over as a prefix and a suffix, one read of the offsets and one copy.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_png.h is: its device entry points have their own memory-discipline matrix
 * (tests/test_gpu_png_file_memory.py) and their own guard (tests/test_png_file_cpu.py).
 */
#ifndef DITHERPIE_HIP_PNG_FILE_H
#define DITHERPIE_HIP_PNG_FILE_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- CRC-32 ----
 *
 * CRC-32/ISO-HDLC: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF (what zlib's crc32 computes).
 * The host statement dp_png_crc32_host_u8 is normative; the device gives the same words for every input.
 *
 * Run r is the sizes[r] bytes at data + r * stride, at any address.  A size outside [0, stride] is the caller's error; it is
 * clamped to that range before it reaches an address computation.
 *
 * How the device cuts a run: into pieces of DP_PNG_CRC_PIECE_BYTES that end on the last 4-byte boundary of the run's
 * addresses, one lane each; a workgroup covers DP_PNG_CRC_SPAN_BYTES in one step.  Pieces and spans are computed
 * independently from a zero register and joined by multiplying with x^(8 * bytes behind them) modulo the polynomial; the
 * bytes a run lacks in front of its first piece count as zeros, the up to three bytes behind the boundary are fed last.
 * The constants are stated for the tests, which aim at those boundaries; the result does not depend on them.
 *
 *   data_dev    n_runs runs, any address
 *   sizes_dev   n_runs int64, 8-byte aligned
 *   crc_dev     n_runs uint32, 4-byte aligned
 *   ws_dev      dp_png_crc32_workspace_bytes(n_runs, stride) bytes, 16-byte aligned; what it held does not matter
 * DP_EINVAL: a NULL pointer, stride < 0 or >= 2^31 - 16, n_runs < 0, a misaligned sizes_dev, crc_dev or ws_dev.
 * DP_EWORKSPACE: ws_bytes too small.  DP_EUNSUPPORTED: n_runs > 65535.  n_runs == 0 returns DP_OK without a launch and
 * touches nothing.  A refused call launches nothing.  dp_png_crc32_workspace_bytes is 0 for arguments that are refused. */
#define DP_PNG_CRC_PIECE_BYTES 64
#define DP_PNG_CRC_SPAN_BYTES 16384
size_t dp_png_crc32_workspace_bytes(int n_runs, int64_t stride);
int dp_png_crc32_u8(const uint8_t *data_dev, int64_t stride, const int64_t *sizes_dev, int n_runs, uint32_t *crc_dev, void *ws_dev,
                    size_t ws_bytes, void *stream);

/* The same on host memory, no device involved (DP_EINVAL as above, without the alignment and workspace rules). */
int dp_png_crc32_host_u8(const uint8_t *data_host, int64_t stride, const int64_t *sizes_host, int n_runs, uint32_t *crc_host);

/* The CRC of A || B from the CRCs of A and B and the length of B (>= 0; a negative length counts as 0). */
uint32_t dp_png_crc32_combine_host(uint32_t crc_a, uint32_t crc_b, int64_t len_b);

/* ---- Finished chunks ----
 *
 * The host statement dp_png_file_assemble_host_u8 is normative; the device writes the same bytes for every input.
 *
 * Input is what dp_png_deflate_encode_u8 (or its _dyn twin) left: frame f's stream is the sizes[f] bytes at
 * streams + f * stream_stride.  A size outside [0, stream_stride] is the caller's error and is clamped to that range first.
 *
 * Frame f of the call becomes, back to back in out:
 *   pre_bytes bytes copied from pre + f * pre_stride   (pre_stride 0: one prefix shared by all frames, else >= pre_bytes;
 *                                                       pre_bytes 0 ... 4096; pre may be NULL when pre_bytes is 0)
 *   ONE chunk: a 4-byte big-endian length, the type, the data, the CRC-32 of type and data, big-endian
 *       f <  n_idat   type IDAT, the data is the stream
 *       f >= n_idat   type fdAT, the data is the big-endian sequence number seq0 + (f - n_idat) * seq_step (modulo 2^32)
 *                     and the stream; the length counts those four bytes
 *   post_bytes bytes copied from post                  (shared by all frames, 0 ... 64; post may be NULL when it is 0)
 * A chunk holds up to 2^31 - 1 bytes, so a stream is never cut into several chunks, and the sequence numbers do not depend
 * on the sizes.  offsets (n_frames + 1 int64, 8-byte aligned) receives the frame boundaries: offsets[0] == 0, frame f is
 * out[offsets[f] ... offsets[f + 1]).  No byte of out at or after offsets[n_frames] is written.
 *
 * dp_png_file_bound_bytes: what no frame exceeds, pre_bytes + 16 + stream_stride + post_bytes.
 * dp_png_file_workspace_bytes: the workspace of the device call.  Both are 0 for arguments that are refused.
 *
 * DP_EINVAL: a NULL streams, sizes, out or offsets (or pre / post with a non-zero length), stream_stride < 0 or
 * >= 2^31 - 16, pre_bytes outside 0 ... 4096, post_bytes outside 0 ... 64, a pre_stride that is neither 0 nor >= pre_bytes,
 * n_frames < 0, n_idat outside 0 ... n_frames, out_bytes < n_frames * dp_png_file_bound_bytes(...), a misaligned sizes_dev,
 * offsets_dev (8 bytes) or ws_dev (16 bytes).  DP_EWORKSPACE: ws_bytes too small.  DP_EUNSUPPORTED: n_frames > 65535.
 * n_frames == 0 returns DP_OK without a launch and touches nothing.  A refused call launches nothing. */
size_t dp_png_file_bound_bytes(int64_t stream_stride, int pre_bytes, int post_bytes);
size_t dp_png_file_workspace_bytes(int n_frames, int64_t stream_stride);
int dp_png_file_assemble_u8(const uint8_t *streams_dev, int64_t stream_stride, const int64_t *sizes_dev, int n_frames, int n_idat,
                            uint32_t seq0, uint32_t seq_step, const uint8_t *pre_dev, int64_t pre_stride, int pre_bytes,
                            const uint8_t *post_dev, int post_bytes, uint8_t *out_dev, size_t out_bytes, int64_t *offsets_dev,
                            void *ws_dev, size_t ws_bytes, void *stream);

/* The same bytes from host memory, no device involved (DP_EINVAL as above, without the alignment and workspace rules). */
int dp_png_file_assemble_host_u8(const uint8_t *streams_host, int64_t stream_stride, const int64_t *sizes_host, int n_frames, int n_idat,
                                 uint32_t seq0, uint32_t seq_step, const uint8_t *pre_host, int64_t pre_stride, int pre_bytes,
                                 const uint8_t *post_host, int post_bytes, uint8_t *out_host, size_t out_bytes, int64_t *offsets_host);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_PNG_FILE_H */
