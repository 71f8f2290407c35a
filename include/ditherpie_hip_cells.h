/*
 * ditherpie_hip_cells.h -- cell-palette dithering with libditherpie_hip.so: the picture is cut into small cells and every cell
 * may show only a few of the palette's colours (two of 15 per 8 x 8 cell on a ZX Spectrum, two of 16 on a C64 in hires, three
 * and a shared background per 4 x 8 cell in its multicolour mode).  Per cell EVERY allowed set of colours is tried on the
 * perturbed pixels and the set of least total error is taken: no quantise-then-repair, no attribute clash.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's
 * current device).  DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason
 * ditherpie_hip_pattern.h is: the test suite pins the device entry points of each header to a memory-discipline matrix; this
 * header has its own (tests/test_gpu_cells_memory.py) and its own guard (tests/test_cells_cpu.py).
 *
 * Definition (all integer arithmetic).
 * Palette: K <= 16 entries whose pal_f32 values lie in [0, 255] (the conditions of ditherpie_hip_pattern.h but for K);
 *   C[j] = trunc(pal_f32[j]) per channel
 *   c    = lut_in[s] per channel for the source bytes s of a pixel (c = s without a lut_in)
 * Cells: cw x ch pixels, each of cw, ch in {4, 8, 16}, anchored at the frame's pixel (0, 0).  Cells on the right and bottom
 *   edge are cut by the frame: only pixels inside the frame count.  Frames of a batch are independent.
 * Perturbation: m in {2, 4, 8}; R the Bayer rank matrix of pattern dithering (B_2 = [[0, 2], [3, 1]],
 *   B_2m = [[4B, 4B + 2], [4B + 3, 4B + 1]]); spread in 0 .. 255.  Per pixel (y, x) and channel
 *     q = clamp(c + floor(((2 R[y mod m][x mod m] + 1 - m*m) * spread) / (2 m*m)), 0, 255)
 *   (floor: an arithmetic shift, 2 m*m is a power of two).
 * Distance: d(p, j) = sum over the channels of (q_p - C[j])^2, at most 195 075.
 * Candidates: colours = k in 1 .. 4; `fixed` a 16-bit mask of entries that every cell owns; 1 .. 4 groups, masks of 16 bits
 *   that may overlap.  The candidates are enumerated group by group in the order the groups are given; within a group the
 *   sets T are the k-subsets of the group's entries that are not in `fixed`, in lexicographic order of their ascending index
 *   tuples; the candidate is S = T | fixed.  At most 4 * C(16, 4) = 7280 candidates.
 * Choice: cost(S) = sum over the pixels p of the cell of min over j in S of d(p, j); below 2^26.  The cell takes the candidate
 *   of least cost, among equal costs the one enumerated first.
 * Output: every pixel of the cell gets out_colors[j] for the j in S of least d(p, j), among equal distances the lowest j.
 *   (Not scipy's tie order: with one group, fixed = 0 and k = K the mode differs from DP_MODE_NEAREST at ties only.)
 *   spread = 0 is nearest-in-S of the unperturbed image.
 * The perturbation also ranks the sets, so the search does not settle on the colour nearest the cell's mean: on a grey ramp
 * of 8 x 8 cells with {black, white}, m = 8 and spread = 255 the number of white pixels per cell rises 0, 2, 4, ... 62.
 */
#ifndef DITHERPIE_HIP_CELLS_H
#define DITHERPIE_HIP_CELLS_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of candidates of a cell for a palette of K entries, or -1 where dp_cells_u8 would return DP_EINVAL for these
 * five: colours outside 1 .. 4, n_groups outside 1 .. 4, a NULL groups_host, a bit of fixed_mask or of a group at or above K,
 * an empty group, a group with fewer than `colours` entries outside fixed_mask -- and for a K outside 1 .. 16, which has no
 * count.  groups_host: n_groups masks in host memory.  Pure host code: no HIP call, no device. */
int dp_cells_candidates(int K, int colours, uint32_t fixed_mask, const uint16_t *groups_host, int n_groups);

/* ---- Cell-palette dithering ----
 *
 *   in_dev/out_dev  n_frames x h x w x 3 uint8, any address.  out_dev == in_dev is allowed (a cell is read whole before any
 *                   of it is written, and cells write only their own bytes); any other overlap is not supported
 *   sets_dev        NULL, or n_frames x ceil(h / ch) x ceil(w / cw) uint16, row-major, 2-byte aligned: the mask of the S each
 *                   cell took, fixed_mask included (what a caller who writes real attribute bytes needs)
 *   groups_host     n_groups masks of HOST memory, read during the call
 *   m, spread       the Bayer matrix size and the spread of the perturbation
 * The call allocates nothing, copies nothing and waits for nothing: it is launches only (the candidates are unranked inside
 * the kernel from a few words of kernel arguments) and legal inside a stream capture from the first call with a palette.  It
 * needs no 2^24 table.  One launch per 65535 frames.  n_frames == 0 (with valid arguments otherwise) returns DP_OK without a
 * launch and touches nothing, in_dev and out_dev may then be NULL.
 * DP_EINVAL: a NULL pointer other than sets_dev, n_frames < 0, h or w < 1, h * w > 2^30, cw or ch outside {4, 8, 16}, m outside
 * {2, 4, 8}, colours or n_groups outside 1 .. 4, spread outside 0 .. 255, a bit of fixed_mask or of a group at or above K, an
 * empty group, a group with fewer than `colours` entries outside fixed_mask, a sets_dev at an odd address.
 * DP_EUNSUPPORTED: K > 16, a palette value outside [0, 255].
 * A refused call launches nothing and names the function in dp_last_error(). */
int dp_cells_u8(const uint8_t *in_dev, uint8_t *out_dev, uint16_t *sets_dev, int64_t n_frames, int h, int w,
                const dp_palette *pal, int cw, int ch, int colours, uint32_t fixed_mask, const uint16_t *groups_host,
                int n_groups, int m, int spread, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_CELLS_H */
