// The address of a colour in a palette's 2^24-entry nearest table (PatDev::tab; built in pattern.hip): 4 x 4 x 4 colours per
// 64-byte line (BRICK), or the plain r | g<<8 | b<<16 order, which only the experiments build fills a table in.  Shared by the
// kernels that gather from the table (pattern.hip, dotdiff.hip) and by a metric palette's top-2 table (metric.hip), which has
// the same brick order with two bytes per colour.
#pragma once
#include <cstdint>

namespace dp {

template <bool BRICK>
__device__ __forceinline__ uint32_t tab_addr(const uint32_t r, const uint32_t g, const uint32_t b)
{
    if (BRICK) return ((r >> 2) << 6) | ((g >> 2) << 12) | ((b >> 2) << 18) | (r & 3u) | ((g & 3u) << 2) | ((b & 3u) << 4);
    return r | (g << 8) | (b << 16);
}

template <bool BRICK>
__device__ __forceinline__ uint32_t tab_colour(const uint32_t a)   // the inverse: r | g<<8 | b<<16 of table address a
{
    if (!BRICK) return a;
    const uint32_t r = (((a >> 6) & 63u) << 2) | (a & 3u), g = (((a >> 12) & 63u) << 2) | ((a >> 2) & 3u),
                   b = (((a >> 18) & 63u) << 2) | ((a >> 4) & 3u);
    return r | (g << 8) | (b << 16);
}

}  // namespace dp
