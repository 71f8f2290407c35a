/*
 * ditherpie_hip_png_dyn.h -- dynamic-Huffman blocks for the PNG-8 output of libditherpie_hip.so: the zlib stream of
 * ditherpie_hip_png.h with one more candidate per segment, a dynamic block (BTYPE 10) over the same tokens.  Opt-in: the
 * entry points of ditherpie_hip_png.h and their bytes are unchanged.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument checks
 * before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's current
 * device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason ditherpie_hip_png.h is:
 * the test suite pins the device entry points of each header to a memory-discipline matrix; this header has its own
 * (tests/test_gpu_png_dyn_memory.py) and its own guard (tests/test_png_dyn_cpu.py).
 */
#ifndef DITHERPIE_HIP_PNG_DYN_H
#define DITHERPIE_HIP_PNG_DYN_H

#include "ditherpie_hip_png.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The stream ----
 *
 * The host statement dp_png_deflate_dyn_host_u8 is normative; the device writes the same bytes for every input.
 *
 * Segments, filtered bytes, matcher, greedy tokens, framing, the realigning block, BFINAL and the Adler-32 are those of
 * ditherpie_hip_png.h.  Per segment there are three candidates: stored, fixed Huffman, and one dynamic block over the same
 * tokens.  The type written is the earliest of the smallest in bytes of the whole segment (stored, fixed, dynamic), the
 * realigning block included.  dp_png_deflate_bound_bytes holds as it is: stored is always a candidate.
 *
 * Histograms: 286 literal/length symbols, symbol 256 (end of block) counted once; 30 distance symbols.
 *
 * Code lengths of an alphabet with counts c[0 .. m) and limit L (15 literal/length, 15 distance, 7 code-length alphabet):
 *   (a) while fewer than two symbols have a count, the lowest-numbered symbol with count 0 gets count 1 (a segment without a
 *       match therefore sends distance codes 0 and 1 with one bit each)
 *   (b) the used symbols ascending by (count, symbol)
 *   (c) a Huffman two-queue merge: when the front leaf's weight is <= the front internal node's weight the leaf is taken;
 *       internal nodes are taken in creation order; a leaf's depth is its length
 *   (d) the limit: num[d] = leaves per depth, depths above L counted at L; total = sum of num[i] << (L - i); while
 *       total > 2^L: num[L]--, for the largest i < L with num[i] > 0: num[i]--, num[i + 1] += 2; total--
 *   (e) lengths from num in sorted order: the first num[L] symbols get L, the next num[L - 1] get L - 1, and so on
 *   (f) canonical codes, RFC 1951 3.2.2
 *
 * Header: HLIT = max(257, the highest literal/length symbol with a length + 1), HDIST = the highest distance symbol with a
 * length + 1.  The two length lists are one sequence (runs may cross the boundary), run-length coded greedily: at a run of r
 * zeros, symbol 18 over min(r, 138) when r >= 11, symbol 17 over r when 3 <= r <= 10, else one literal 0; at a run of a
 * length v, the literal v, then symbol 16 over min(rest, 6) while the rest is >= 3 (a rest of 1 or 2 is coded by the next
 * rounds as literals).  The code-length alphabet's code is rules (a) ... (f) with L = 7 over the counts of symbols 0 ... 18;
 * HCLEN = max(4, 1 + the last index of RFC 1951's order whose symbol has a length).
 *
 * Size: the block's bits from its three header bits through end-of-block follow from the histograms, the total of extra bits
 * and the code lengths alone; they are known before a bit is written.
 *
 * Arguments, refusals and n_frames == 0 as dp_png_deflate_encode_u8 / dp_png_deflate_host_u8.  The workspace is larger than
 * dp_png_deflate_workspace_bytes: it also holds one 32-bit word per token (4 * min(seg_bytes, F) bytes per segment). */
size_t dp_png_deflate_dyn_workspace_bytes(int n_frames, int h, int w, int depth, int seg_bytes);
int dp_png_deflate_dyn_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_dev,
                                 int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream);
int dp_png_deflate_dyn_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_host,
                               int64_t out_stride, int64_t *sizes_host);

/* Rules (a) ... (e) on their own: n_alphabets histograms of n_symbols uint32 counts back to back -> n_alphabets lists of
 * n_symbols one-byte lengths, one wave per histogram.  Exported because the 15-bit limit of (d) is out of reach of a stream a
 * test can afford; the code is the one the encoder runs.
 * DP_EINVAL: a NULL pointer, n_alphabets < 0, n_symbols outside 2 ... 286, max_len outside 1 ... 15, 2^max_len < n_symbols,
 * a misaligned counts_dev (4 bytes), and, on the host, a count above 2^20.  The device entry point cannot see the counts
 * before the launch: there a count above 2^20 is the caller's error and is taken as 2^20.  n_alphabets == 0 returns DP_OK and
 * touches nothing.  No workspace. */
int dp_png_code_lengths_u8(const uint32_t *counts_dev, int n_alphabets, int n_symbols, int max_len, uint8_t *lengths_dev, void *stream);
int dp_png_code_lengths_host(const uint32_t *counts_host, int n_alphabets, int n_symbols, int max_len, uint8_t *lengths_host);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_PNG_DYN_H */
