// The hand-scheduled candidate networks of the ordered kernels (ordered.hip, which alone includes this): keys of the 4, 6 or 8
// candidates of a pixel and the two or three smallest of them.
//   key = ((|p|^2 - 2 x.p) << 8) | (4*idx)      (4*idx = byte offset of the candidate inside its block)
// Hand scheduled: hipcc neither fuses the shift/add/multiply into v_lshl_add + v_mad_i32_i24 nor keeps med3 for the running
// top-3, and it has to pad DOT results with s_nop; here all v_dot4 are issued first (a DOT result must not be read for 3 issue
// slots), then the keys, then the smallest: sort the first three (min3/med3/max3), insert the others.
//
// Every network is put together from the thirteen instruction lines below, one string macro each (as DP_STEP4 in
// wave_util.hip.h), so that a network reads as its recipe and a new one is not forty copied lines with edited digits.  The
// operands are named: x the pixel, c_j the colour of candidate j, k_j its staged norm (|c_j|^2 << 8) + 4 j, n_j its key (and
// the norm on the way there), p_j the dot product x.c_j, m0 <= m1 <= m2 the smallest keys, ng = -512.
#pragma once
#include "dp_internal.h"

namespace dp {

// ---- the vocabulary -----------------------------------------------------------------------------------------------------
#define DPC_NORM(j) "v_dot4_u32_u8 %[n" #j "], %[c" #j "], %[c" #j "], 0\n\t"            /* n_j = c_j . c_j */
#define DPC_PDOT(j) "v_dot4_u32_u8 %[p" #j "], %[x], %[c" #j "], 0\n\t"                  /* p_j = x . c_j */
#define DPC_NDOT(j) "v_dot4_u32_u8 %[n" #j "], %[x], %[c" #j "], 0\n\t"                  /* n_j = x . c_j (cand8r) */
#define DPC_SLOT(j, at) "v_lshl_add_u32 %[n" #j "], %[n" #j "], 8, " #at "\n\t"          /* n_j = (n_j << 8) + at, at = 4 j */
#define DPC_KEY(j) "v_mad_i32_i24 %[n" #j "], %[p" #j "], %[ng], %[n" #j "]\n\t"         /* n_j = p_j * ng + n_j */
#define DPC_KEY_PK(j) "v_mad_i32_i24 %[n" #j "], %[p" #j "], %[ng], %[k" #j "]\n\t"      /* n_j = p_j * ng + k_j */
#define DPC_KEY_NK(j) "v_mad_i32_i24 %[n" #j "], %[n" #j "], %[ng], %[k" #j "]\n\t"      /* n_j = n_j * ng + k_j */
#define DPC_MIN3 "v_min3_i32 %[m0], %[n0], %[n1], %[n2]\n\t"
#define DPC_MED3 "v_med3_i32 %[m1], %[n0], %[n1], %[n2]\n\t"
#define DPC_MAX3 "v_max3_i32 %[m2], %[n0], %[n1], %[n2]\n\t"
#define DPC_INS2(j) "v_med3_i32 %[m2], %[m1], %[m2], %[n" #j "]\n\t"                     /* n_j into m2 */
#define DPC_INS1(j) "v_med3_i32 %[m1], %[m0], %[m1], %[n" #j "]\n\t"                     /* ... into m1 */
#define DPC_INS0(j) "v_min_i32 %[m0], %[m0], %[n" #j "]\n\t"                             /* ... into m0 */

// ---- groups -------------------------------------------------------------------------------------------------------------
#define DPC_DOTS(j) DPC_NORM(j) DPC_PDOT(j)
#define DPC_DOTS03 DPC_DOTS(0) DPC_DOTS(1) DPC_DOTS(2) DPC_DOTS(3)                 // both dots of entries 0-3
#define DPC_DOTS45 DPC_DOTS(4) DPC_DOTS(5)
#define DPC_DOTS67 DPC_DOTS(6) DPC_DOTS(7)
#define DPC_PDOTS03 DPC_PDOT(0) DPC_PDOT(1) DPC_PDOT(2) DPC_PDOT(3)                // pixel dots only: the norms are staged
#define DPC_KEYS03 DPC_SLOT(0, 0) DPC_SLOT(1, 4) DPC_SLOT(2, 8) DPC_SLOT(3, 12) DPC_KEY(0) DPC_KEY(1) DPC_KEY(2) DPC_KEY(3)
#define DPC_KEYS05 DPC_SLOT(0, 0) DPC_SLOT(1, 4) DPC_SLOT(2, 8) DPC_SLOT(3, 12) DPC_SLOT(4, 16) DPC_SLOT(5, 20) \
    DPC_KEY(0) DPC_KEY(1) DPC_KEY(2) DPC_KEY(3) DPC_KEY(4) DPC_KEY(5)
#define DPC_KEYS07 DPC_SLOT(0, 0) DPC_SLOT(1, 4) DPC_SLOT(2, 8) DPC_SLOT(3, 12) DPC_SLOT(4, 16) DPC_SLOT(5, 20) DPC_SLOT(6, 24) DPC_SLOT(7, 28) \
    DPC_KEY(0) DPC_KEY(1) DPC_KEY(2) DPC_KEY(3) DPC_KEY(4) DPC_KEY(5) DPC_KEY(6) DPC_KEY(7)
#define DPC_KEYS45 DPC_SLOT(4, 16) DPC_SLOT(5, 20) DPC_KEY(4) DPC_KEY(5)
#define DPC_KEYS_PK03 DPC_KEY_PK(0) DPC_KEY_PK(1) DPC_KEY_PK(2) DPC_KEY_PK(3)      // keys 0-3 from staged norms
#define DPC_SORT3 DPC_MIN3 DPC_MED3 DPC_MAX3                                       // m0 <= m1 <= m2 of n0..n2
#define DPC_SORT2 DPC_MIN3 DPC_MED3                                                // m0 <= m1 only
#define DPC_TOP3(j) DPC_INS2(j) DPC_INS1(j) DPC_INS0(j)                            // insert n_j into the top three
#define DPC_TOP2(j) DPC_INS1(j) DPC_INS0(j)                                        // ... into the top two

// ---- operand lists ------------------------------------------------------------------------------------------------------
#define DPC_O(r) [r] "=&v"(r)
#define DPC_I(name, v) [name] "v"(v)
#define DPC_O4(a) DPC_O(a##0), DPC_O(a##1), DPC_O(a##2), DPC_O(a##3)
#define DPC_O6(a) DPC_O4(a), DPC_O(a##4), DPC_O(a##5)
#define DPC_O8(a) DPC_O6(a), DPC_O(a##6), DPC_O(a##7)
#define DPC_OM2 DPC_O(m0), DPC_O(m1)
#define DPC_OM3 DPC_OM2, DPC_O(m2)
#define DPC_I4(a, j0, j1, j2, j3, v) DPC_I(a##j0, v.x), DPC_I(a##j1, v.y), DPC_I(a##j2, v.z), DPC_I(a##j3, v.w)
#define DPC_NG [ng] "s"(neg2)

// Keys of the 8 candidates of one block and the three smallest of them: all eight v_dot4 pairs first, then 2 ops per key, then
// the three smallest: sort the first three, insert the other five (3 ops each).  `neg2` = -512 must sit in an SGPR (v_mad_i32_i24 takes no literal).
__device__ __forceinline__ void cand8(const uint32_t x, const uint4 ca, const uint4 cb, const int neg2, int &m0,
                                      int &m1, int &m2)
{
    int n0, n1, n2, n3, n4, n5, n6, n7, p0, p1, p2, p3, p4, p5, p6, p7;
    asm volatile(DPC_DOTS03 DPC_DOTS45 DPC_DOTS67 DPC_KEYS07 DPC_SORT3 DPC_TOP3(3) DPC_TOP3(4) DPC_TOP3(5) DPC_TOP3(6) DPC_TOP3(7)
                 : DPC_O8(n), DPC_O8(p), DPC_OM3
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I4(c, 4, 5, 6, 7, cb), DPC_NG);
}

// The same keys, the TWO smallest only (pixels that take their nearest entry whatever the second one is): 44 operations
__device__ __forceinline__ void cand8n(const uint32_t x, const uint4 ca, const uint4 cb, const int neg2, int &m0, int &m1)
{
    int n0, n1, n2, n3, n4, n5, n6, n7, p0, p1, p2, p3, p4, p5, p6, p7;
    asm volatile(DPC_DOTS03 DPC_DOTS45 DPC_DOTS67 DPC_KEYS07 DPC_SORT2 DPC_TOP2(3) DPC_TOP2(4) DPC_TOP2(5) DPC_TOP2(6) DPC_TOP2(7)
                 : DPC_O8(n), DPC_O8(p), DPC_OM2
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I4(c, 4, 5, 6, 7, cb), DPC_NG);
}

// Keys of the 4 candidates of a small block and the three smallest (see cand8)
__device__ __forceinline__ void cand4(const uint32_t x, const uint4 ca, const int neg2, int &m0, int &m1, int &m2)
{
    int n0, n1, n2, n3, p0, p1, p2, p3;
    asm volatile(DPC_DOTS03 DPC_KEYS03 DPC_SORT3 DPC_TOP3(3)
                 : DPC_O4(n), DPC_O4(p), DPC_OM3
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_NG);
}

// keys of eight palette records and the three smallest (see cand8); r_k = {colour, |p|^2 << 8 | index}
__device__ __forceinline__ void cand8r(const uint32_t x, const uint2 r0, const uint2 r1, const uint2 r2, const uint2 r3,
                                       const uint2 r4, const uint2 r5, const uint2 r6, const uint2 r7, const int neg2, int &m0,
                                       int &m1, int &m2)
{
    int n0, n1, n2, n3, n4, n5, n6, n7;
    asm volatile(DPC_NDOT(0) DPC_NDOT(1) DPC_NDOT(2) DPC_NDOT(3) DPC_NDOT(4) DPC_NDOT(5) DPC_NDOT(6) DPC_NDOT(7)
                 DPC_KEY_NK(0) DPC_KEY_NK(1) DPC_KEY_NK(2) DPC_KEY_NK(3) DPC_KEY_NK(4) DPC_KEY_NK(5) DPC_KEY_NK(6) DPC_KEY_NK(7)
                 DPC_SORT3 DPC_TOP3(3) DPC_TOP3(4) DPC_TOP3(5) DPC_TOP3(6) DPC_TOP3(7)
                 : DPC_O8(n), DPC_OM3
                 : DPC_I(x, x), DPC_I(c0, r0.x), DPC_I(c1, r1.x), DPC_I(c2, r2.x), DPC_I(c3, r3.x), DPC_I(c4, r4.x), DPC_I(c5, r5.x),
                   DPC_I(c6, r6.x), DPC_I(c7, r7.x), DPC_I(k0, r0.y), DPC_I(k1, r1.y), DPC_I(k2, r2.y), DPC_I(k3, r3.y), DPC_I(k4, r4.y),
                   DPC_I(k5, r5.y), DPC_I(k6, r6.y), DPC_I(k7, r7.y), DPC_NG);
}

// byte k of `word` times 8 (the LDS address of palette record number byte k): one SDWA shift; `three` holds 3
template <int BYTE>
__device__ __forceinline__ uint32_t rec_addr(const uint32_t word, const uint32_t three)
{
#define DPC_REC_ADDR(k) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #k : "=v"(a) : "v"(three), "v"(word))
    uint32_t a;
    if (BYTE == 0) DPC_REC_ADDR(0);
    else if (BYTE == 1) DPC_REC_ADDR(1);
    else if (BYTE == 2) DPC_REC_ADDR(2);
    else DPC_REC_ADDR(3);
    return a;
#undef DPC_REC_ADDR
}

// Keys of the first six entries of a block and the two smallest (see cand8)
__device__ __forceinline__ void cand6n(const uint32_t x, const uint4 ca, const uint32_t c4, const uint32_t c5, const int neg2,
                                       int &m0, int &m1)
{
    int n0, n1, n2, n3, n4, n5, p0, p1, p2, p3, p4, p5;
    asm volatile(DPC_DOTS03 DPC_DOTS45 DPC_KEYS05 DPC_SORT2 DPC_TOP2(3) DPC_TOP2(4) DPC_TOP2(5)
                 : DPC_O6(n), DPC_O6(p), DPC_OM2
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I(c4, c4), DPC_I(c5, c5), DPC_NG);
}

// The same for the four entries of a small block
__device__ __forceinline__ void cand4n(const uint32_t x, const uint4 ca, const int neg2, int &m0, int &m1)
{
    int n0, n1, n2, n3, p0, p1, p2, p3;
    asm volatile(DPC_DOTS03 DPC_KEYS03 DPC_SORT2 DPC_TOP2(3)
                 : DPC_O4(n), DPC_O4(p), DPC_OM2
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_NG);
}

// Keys of the six candidates of a window and the three smallest (see cand8)
__device__ __forceinline__ void cand6(const uint32_t x, const uint4 ca, const uint32_t c4, const uint32_t c5, const int neg2, int &m0,
                                      int &m1, int &m2)
{
    int n0, n1, n2, n3, n4, n5, p0, p1, p2, p3, p4, p5;
    asm volatile(DPC_DOTS03 DPC_DOTS45 DPC_KEYS05 DPC_SORT3 DPC_TOP3(3) DPC_TOP3(4) DPC_TOP3(5)
                 : DPC_O6(n), DPC_O6(p), DPC_OM3
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I(c4, c4), DPC_I(c5, c5), DPC_NG);
}

// Key levels 1 and 2 (ordered_fine.h: fine_keys_level): the part of a key that does not depend on the pixel, N_j = (|c_j|^2 << 8)
// + 4 j, is staged in LDS next to the colour, and a key is two instructions -- the same value as cand4n / cand6 compute with four.
// cand4k: keys of the quad A from its norms na, and the two smallest
__device__ __forceinline__ void cand4k(const uint32_t x, const uint4 ca, const uint4 na, const int neg2, int &m0, int &m1)
{
    int n0, n1, n2, n3, p0, p1, p2, p3;
    asm volatile(DPC_PDOTS03 DPC_KEYS_PK03 DPC_SORT2 DPC_TOP2(3)
                 : DPC_O4(n), DPC_O4(p), DPC_OM2
                 : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I4(k, 0, 1, 2, 3, na), DPC_NG);
}

// cand6k: keys of the six candidates of a window and the three smallest.  KEYS 1: the pair B comes as colours only (c4, c5; its two
// keys take four instructions as in cand6); KEYS 2: with its norms k4, k5.
template <int KEYS>
__device__ __forceinline__ void cand6k(const uint32_t x, const uint4 ca, const uint4 na, const uint32_t c4, const uint32_t c5,
                                       const uint32_t k4, const uint32_t k5, const int neg2, int &m0, int &m1, int &m2)
{
    int n0, n1, n2, n3, n4, n5, p0, p1, p2, p3, p4, p5;
    if constexpr (KEYS == 1) {
        (void)k4, (void)k5;
        asm volatile(DPC_PDOTS03 DPC_DOTS45 DPC_KEYS_PK03 DPC_KEYS45 DPC_SORT3 DPC_TOP3(3) DPC_TOP3(4) DPC_TOP3(5)
                     : DPC_O6(n), DPC_O6(p), DPC_OM3
                     : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I(c4, c4), DPC_I(c5, c5), DPC_I4(k, 0, 1, 2, 3, na), DPC_NG);
    } else {
        asm volatile(DPC_PDOTS03 DPC_PDOT(4) DPC_PDOT(5) DPC_KEYS_PK03 DPC_KEY_PK(4) DPC_KEY_PK(5) DPC_SORT3 DPC_TOP3(3) DPC_TOP3(4) DPC_TOP3(5)
                     : DPC_O6(n), DPC_O6(p), DPC_OM3
                     : DPC_I(x, x), DPC_I4(c, 0, 1, 2, 3, ca), DPC_I(c4, c4), DPC_I(c5, c5), DPC_I4(k, 0, 1, 2, 3, na), DPC_I(k4, k4),
                       DPC_I(k5, k5), DPC_NG);
    }
}

}  // namespace dp
