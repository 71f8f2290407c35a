/*
 * ditherpie_hip_indexed.h -- indexed output of libditherpie_hip.so: palette-index planes beside packed RGB.
 *
 * Every dither mode writes, per pixel, one of the K <= DP_MAX_COLORS output colours of its palette, so a dithered frame
 * is a palette image; the entry points below convert between its two forms on the device.  An extension of
 * ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument checks before any
 * HIP call, `stream` a hipStream_t passed as void*, work enqueued asynchronously, the calling thread's current device).
 * DP_ABI_VERSION is unchanged: these are additions.  The functions live in a header of their own because the test
 * suite pins the list of device entry points of ditherpie_hip.h to its memory-discipline matrix; this header has its
 * own matrix (tests/test_gpu_indexed_memory.py) and its own guard (tests/test_indexed_cpu.py).
 *
 * Contract.  For a list of K output colours C[0..K) (uint8 RGB, duplicates allowed) and an RGB pixel p:
 *   - index(p) is the LOWEST j with C[j] == p;
 *   - a pixel equal to no entry is MISSING: it gets index 0 and is counted, and the count is exact;
 *   - decode(index(p)) == p for every pixel that is not missing.  Where C has duplicates (use_gamma palettes whose sRGB
 *     forms collide, palettes with repeated entries) the index is therefore the lowest of the equal entries, not
 *     necessarily the entry the nearest-colour search chose: the RGB output cannot tell them apart either;
 *   - an index plane holds one byte per pixel for K <= 256, or two bytes (little-endian, values < K) for any K; the
 *     caller chooses (index_bytes), one byte is refused for K > 256.  Planes are h x w, row pitch w * index_bytes,
 *     frames back to back -- the entry points take the pixel count only.
 */
#ifndef DITHERPIE_HIP_INDEXED_H
#define DITHERPIE_HIP_INDEXED_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dp_index_map dp_index_map; /* colour -> index table + index -> colour list, library-owned */

/* dp_index_map_create: colors_host is K x 3 uint8 (the out_colors of a palette), 1 <= K <= DP_MAX_COLORS.  Builds, on
 * the host, an open-addressing hash table of 2048 (K <= 512) or 4096 four-byte slots with a multiplier chosen so that
 * no entry lies more than 6 slots from its home (DP_EUNSUPPORTED if no multiplier achieves it).  No HIP call: the first
 * launch with the map uploads the table and the colour list to the current device (20 KB, synchronous, once, under the
 * map's mutex); the map then belongs to that device and is refused (DP_EINVAL) on another.
 * dp_index_map_info: K, the number of slots and the longest displacement (any pointer may be NULL).
 * dp_index_map_destroy: frees the device copy; the caller makes sure no launch with the map is still in flight. */
int dp_index_map_create(const uint8_t *colors_host, int K, dp_index_map **out);
void dp_index_map_destroy(dp_index_map *map);
int dp_index_map_info(const dp_index_map *map, int *K, int *slots, int *max_probe);

/* RGB frames -> index plane.
 *   rgb_dev        n_px packed RGB pixels (3 * n_px bytes), any address
 *   index_dev      n_px indices of index_bytes bytes each (1 or 2); a 2-byte plane at an even address
 *   n_missing_dev  one int64 on the device, 8-byte aligned: the number of missing pixels is ADDED to it (the caller
 *                  zeroes it; several calls may accumulate into one counter)
 * One launch: the table in LDS, four pixels per lane as one 12-byte load and one 4- (8-) byte store where rgb_dev is
 * 4-byte and index_dev 4- (8-) byte aligned, one pixel per lane otherwise and for the last n_px % 4 pixels.
 * DP_EINVAL: a NULL pointer, n_px < 0, index_bytes not 1 or 2, index_bytes 1 with K > 256, a 2-byte plane at an odd
 * address, a counter that is not 8-byte aligned.  n_px == 0 returns DP_OK without a launch. */
int dp_index_from_rgb_u8(const uint8_t *rgb_dev, void *index_dev, int64_t n_px, const dp_index_map *map, int index_bytes,
                         int64_t *n_missing_dev, void *stream);

/* Index plane -> RGB frames (the inverse).  An index >= K is written as entry 0 and counted into *n_bad_dev (added,
 * as above).  Same layout, alignment rules and refusals as dp_index_from_rgb_u8. */
int dp_rgb_from_index_u8(const void *index_dev, uint8_t *rgb_dev, int64_t n_px, const dp_index_map *map, int index_bytes,
                         int64_t *n_bad_dev, void *stream);

/* NEAREST resize of index planes (or any planes of 1- or 2-byte elements): n_frames x h x w -> n_frames x oh x ow with
 * the source coordinates of dp_resize_nearest_u8 (Pillow's double-accumulated tables), so resizing the plane and
 * decoding equals decoding and resizing.  DP_EINVAL: a NULL pointer, a size < 1 (n_frames == 0 returns DP_OK without a
 * launch), elem_bytes not 1 or 2, a 2-byte plane at an odd address.  DP_EUNSUPPORTED: oh or n_frames > 65535. */
int dp_resize_nearest_plane_u8(const void *in_dev, void *out_dev, int64_t n_frames, int h, int w, int oh, int ow,
                               int elem_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_INDEXED_H */
