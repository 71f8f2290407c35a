// The device statement of (L, a, b) under the Oklab metric (include/ditherpie_hip_metric.h), shared by metric.hip and okfit.hip:
// the LIN literal in constant memory (each translation unit that includes this has its own copy), the exact integer cube root and
// lab_dev.  metric.hip's header comment has the derivation of the cube root.
#pragma once
#include "dp_internal.h"

namespace dp {
namespace {

__constant__ uint16_t c_lin[256] = {DP_METRIC_LIN_VALUES};

template <bool TAB>
__device__ __forceinline__ int icbrt_dev(const uint32_t x, const uint16_t *__restrict__ cbrt_tab)
{
    if (TAB) return (int)cbrt_tab[x];
    // cbrt(x 2^32) = 2^(log2(x) / 3 + 32 / 3); x = 0: log2 is -inf, exp2 of it 0
    uint32_t c = (uint32_t)__builtin_amdgcn_exp2f(__builtin_amdgcn_logf((float)x) * (1.0f / 3.0f) + (32.0f / 3.0f));
    c = min(c, 65535u);
    // c^3 against x << 32: the high word of the 48-bit cube decides, the low word only at equality
    const uint32_t c2 = c * c;
    if (__umulhi(c2, c) > x || (__umulhi(c2, c) == x && c2 * c != 0u)) --c;
    const uint32_t n = c + 1u, n2 = n * n;   // n = 65536 (n2 wraps) is never the root: 65536^3 > 65535 << 32
    if (n <= 65535u && (__umulhi(n2, n) < x || (__umulhi(n2, n) == x && n2 * n == 0u))) c = n;
    return (int)c;
}

// THE device statement of (L, a, b): s_lin is LIN (in LDS)
template <bool TAB>
__device__ __forceinline__ void lab_dev(const uint32_t r, const uint32_t g, const uint32_t b, const uint16_t *s_lin,
                                        const uint16_t *__restrict__ cbrt_tab, int &L, int &A, int &B)
{
    const uint32_t lr = s_lin[r], lg = s_lin[g], lb = s_lin[b];
    const int cl = icbrt_dev<TAB>((27015u * lr + 35149u * lg + 3372u * lb) >> 16, cbrt_tab);
    const int cm = icbrt_dev<TAB>((13887u * lr + 44611u * lg + 7038u * lb) >> 16, cbrt_tab);
    const int cs = icbrt_dev<TAB>((5787u * lr + 18463u * lg + 41286u * lb) >> 16, cbrt_tab);
    L = (862 * cl + 3251 * cm - 17 * cs) >> 14;       // arithmetic shifts: floor
    A = (8102 * cl - 9948 * cm + 1846 * cs) >> 14;
    B = (106 * cl + 3206 * cm - 3312 * cs) >> 14;
}

}  // namespace
}  // namespace dp
