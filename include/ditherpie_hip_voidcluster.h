/*
 * ditherpie_hip_voidcluster.h -- void-and-cluster threshold matrices (Ulichney 1993) with libditherpie_hip.so: blue-noise rank
 * matrices that tile, generated on the device.  dp_thresholds_blue_noise reproduces the reference's generator, a
 * farthest-point ordering on a square that does not wrap, whose matrix is white noise above mid grey; this is the generator
 * to use when the quality of the mask matters.  The result is an ordinary dp_thresholds for DP_MODE_MATRIX.
 *
 * An extension of ditherpie_hip.h (same library, same conventions: 0 / DP_E* status codes, dp_last_error(), argument
 * checks before any HIP call, `stream` a hipStream_t passed as void*, the calling thread's current device).
 * DP_ABI_VERSION is unchanged: these are additions.  A header of its own for the reason ditherpie_hip_dotdiff.h is: the test
 * suite pins the device entry points of each header to a memory-discipline matrix; this header has its own
 * (tests/test_gpu_voidcluster_memory.py) and its own guard (tests/test_voidcluster_cpu.py).
 *
 * Definition (all integer arithmetic; tests/vac_ref.py states it in numpy).  h, w in 8 .. 128, n = h * w; seed a uint32;
 * sigma256 in 256 .. 768, sigma = sigma256 / 256.
 *   W[d2]   = floor(exp(-(d2 * 32768.0) / (sigma256 * sigma256)) * 2^20 + 0.5)    in double on the host; zero beyond some D
 *             (D = 29 at sigma256 256, 65 at 384, 116 at 512, 262 at 768)
 *   T(p, q) = W[a^2 + b^2],  a = min(|dy| mod h, h - |dy| mod h), b likewise in x: the minimum image on the torus, counted
 *             once even where the window of W is wider than the matrix
 *   E[p]    = the sum of T(p, q) over the set cells q                                  (at most 59 295 600)
 * In every choice below the lowest row-major index wins a tie.
 *   1. mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32)
 *   2. key(i) = mix32(mix32(i) ^ seed); n1 = max(1, n / 10); the n1 cells of the smallest (key, i) are set
 *   3. relax, at most 4 n rounds: clear c, the set cell of the largest E; set v, the unset cell of the smallest E; stop after
 *      the round in which v == c.  The pattern reached is the prototype
 *   4. from the prototype, for r = n1 - 1 down to 0: clear the set cell of the largest E, its rank is r.  (E is zero after.)
 *   5. from the prototype again, for r = n1 .. n - 1: set the unset cell of the smallest E, its rank is r
 *   6. thresholds: L = min(n, 4096), t = float32((2 floor(rank L / n) + 1) / (2 L)): bin centres, all inside (0, 1).  With
 *      power-of-two sizes every t is a multiple of 2^-13 and the matrix takes the integer form of the ordered kernels.
 */
#ifndef DITHERPIE_HIP_VOIDCLUSTER_H
#define DITHERPIE_HIP_VOIDCLUSTER_H

#include "ditherpie_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DP_VOID_CLUSTER_MIN_SIZE 8
#define DP_VOID_CLUSTER_MAX_SIZE 128
#define DP_VOID_CLUSTER_MIN_SIGMA256 256
#define DP_VOID_CLUSTER_MAX_SIGMA256 768

/* Rank matrices on the device: ranks_dev receives n_matrices x h x w uint16 (2-byte aligned), matrix i generated from
 * seeds_host[i] (HOST memory, read during the call).  One workgroup per matrix runs steps 2 to 5 in one launch; the weights
 * travel to the kernel by value.  Launches only: no allocation, no copy, no synchronisation, so a call may be captured into
 * a graph from the first one on.  n_matrices == 0 returns DP_OK and touches nothing (the pointers may then be NULL).
 * DP_EINVAL: a NULL pointer, n_matrices < 0, h or w outside 8 .. 128, sigma256 outside 256 .. 768.  A refused call launches
 * nothing and names the function in dp_last_error(). */
int dp_void_cluster_u16(uint16_t *ranks_dev, int n_matrices, const uint32_t *seeds_host, int h, int w, int sigma256,
                        void *stream);

/* The same matrix computed on the host: ranks_host receives h x w uint16.  Pure host code: no HIP call, no device.
 * DP_EINVAL as above. */
int dp_void_cluster_host(uint16_t *ranks_host, int h, int w, uint32_t seed, int sigma256);

/* The dp_thresholds_blue_noise counterpart: generates the matrix on the device, downloads it, applies step 6 and builds the
 * dp_thresholds (integer form and padded table included).  Unlike dp_void_cluster_u16 it ALLOCATES device memory and
 * SYNCHRONISES the stream (and no other: its copies run on `stream`, not on the null stream): not for use inside a
 * graph capture.  Free the result with dp_thresholds_destroy.
 * DP_EINVAL: out == NULL or a size or sigma256 out of range, before any HIP call. */
int dp_thresholds_void_cluster(int h, int w, uint32_t seed, int sigma256, void *stream, dp_thresholds **out);

#ifdef __cplusplus
}
#endif
#endif /* DITHERPIE_HIP_VOIDCLUSTER_H */
