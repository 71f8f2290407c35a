// Indexed output (include/ditherpie_hip_indexed.h): RGB frames <-> palette-index planes, and the NEAREST resize of planes.
//
// index_from_rgb_kernel   the colour -> index hash table of host_logic.h (index_map_build) in LDS; 3 B read and 1 (2) B
//                         written per pixel.  Four pixels per lane where the addresses allow it: one 12-byte load, four
//                         bounded probe runs, one 4- (8-) byte store; otherwise, and for the last n_px % 4 pixels, one pixel
//                         per lane.  Missing pixels are counted per lane and added to the caller's counter once per wave
//                         that saw any.
// rgb_from_index_kernel   the inverse: the K colours in LDS, 1 (2) B read and 3 B written per pixel, same two shapes.
// plane_resize_kernel     out[f][y][x] = in[f][ytab[y]][xtab[x]] with Pillow's coordinate tables (restated from ordered.hip:
//                         the RGB instance there is left as it is).
#include "dp_internal.h"
#include "wave_util.hip.h"

#include "../../include/ditherpie_hip_indexed.h"

struct dp_index_map {
    dp::IndexMapHost host;
    // the device copy (table[slots] | colors[K], one allocation) is made by the first launch, under mu
    mutable std::mutex mu;
    mutable void *blob = nullptr;
    mutable int device = -1;
};

namespace dp {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;   // 8 blocks of 256 threads per CU; the rest of the work by grid stride

struct IndexMapDev {
    const uint32_t *table;
    const uint32_t *colors;
    int K, slots, rest_bits, max_probe;
    uint32_t mult;
};

struct alignas(4) Word3 {
    uint32_t x, y, z;
};

// host_logic.h: index_map_lookup, on the LDS copy.  A colour is stored once, so at most one step of the run matches; the
// run has the map's own longest displacement + 1 steps (wave-uniform) and does not look for empty slots.
__device__ __forceinline__ uint32_t map_find(const uint32_t *tab, const uint32_t c, const IndexMapDev &m, const uint32_t slot_mask,
                                             uint32_t &miss)
{
    const uint32_t h = (c * m.mult) & 0xFFFFFFu;
    const uint32_t home = h >> m.rest_bits;
    uint32_t want = h & ((1u << m.rest_bits) - 1u);
    uint32_t idx = 0, found = 0;
    for (int d = 0; d <= m.max_probe; ++d) {
        const uint32_t w = tab[(home + (uint32_t)d) & slot_mask];
        const bool hit = (w & 0xFFFFu) == want;
        idx = hit ? (w >> 16) : idx;
        found |= hit ? 1u : 0u;
        want += 1u << 13;
    }
    miss += found ^ 1u;
    return idx;
}

// every lane of the block arrives here (no early exit above): one atomic per wave that counted anything
__device__ __forceinline__ void add_to_counter(unsigned long long *counter, const uint32_t n)
{
    if (__ballot(n != 0) == 0) return;
    const uint32_t total = wave_sum_to_lane63(n);
    if ((threadIdx.x & 63) == 63) atomicAdd(counter, (unsigned long long)total);
}

template <int BYTES>
__device__ __forceinline__ void store_index(void *index, const long long i, const uint32_t v)
{
    if (BYTES == 1)
        static_cast<uint8_t *>(index)[i] = (uint8_t)v;
    else
        static_cast<uint16_t *>(index)[i] = (uint16_t)v;
}

template <int BYTES>
__device__ __forceinline__ uint32_t load_index(const void *index, const long long i)
{
    return BYTES == 1 ? (uint32_t) static_cast<const uint8_t *>(index)[i] : (uint32_t) static_cast<const uint16_t *>(index)[i];
}

// VEC: rgb is 4-byte aligned and index 4 * BYTES-byte aligned
template <int BYTES, bool VEC>
__global__ __launch_bounds__(kBlock) void index_from_rgb_kernel(const uint8_t *__restrict__ rgb, void *__restrict__ index,
                                                                const long long n_px, const IndexMapDev m,
                                                                unsigned long long *__restrict__ n_missing)
{
    __shared__ uint32_t tab[kIndexMapMaxSlots];
    for (int i = threadIdx.x; i < m.slots; i += kBlock) tab[i] = m.table[i];
    __syncthreads();
    const uint32_t slot_mask = (uint32_t)m.slots - 1u;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    uint32_t miss = 0;
    long long scalar_from = 0;
    if (VEC) {
        const long long n4 = n_px >> 2;
        for (long long g = gid; g < n4; g += stride) {
            const Word3 p = reinterpret_cast<const Word3 *>(rgb)[g];
            const uint32_t i0 = map_find(tab, p.x & 0xFFFFFFu, m, slot_mask, miss);
            const uint32_t i1 = map_find(tab, (p.x >> 24) | ((p.y & 0xFFFFu) << 8), m, slot_mask, miss);
            const uint32_t i2 = map_find(tab, (p.y >> 16) | ((p.z & 0xFFu) << 16), m, slot_mask, miss);
            const uint32_t i3 = map_find(tab, p.z >> 8, m, slot_mask, miss);
            if (BYTES == 1)
                static_cast<uint32_t *>(index)[g] = i0 | (i1 << 8) | (i2 << 16) | (i3 << 24);
            else
                static_cast<uint2 *>(index)[g] = make_uint2(i0 | (i1 << 16), i2 | (i3 << 16));
        }
        scalar_from = n4 << 2;
    }
    for (long long i = scalar_from + gid; i < n_px; i += stride) {
        const uint8_t *p = rgb + 3 * i;
        const uint32_t c = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        store_index<BYTES>(index, i, map_find(tab, c, m, slot_mask, miss));
    }
    add_to_counter(n_missing, miss);
}

template <int BYTES, bool VEC>
__global__ __launch_bounds__(kBlock) void rgb_from_index_kernel(const void *__restrict__ index, uint8_t *__restrict__ rgb,
                                                                const long long n_px, const IndexMapDev m,
                                                                unsigned long long *__restrict__ n_bad)
{
    __shared__ uint32_t pal[DP_MAX_COLORS];
    for (int i = threadIdx.x; i < m.K; i += kBlock) pal[i] = m.colors[i];
    __syncthreads();
    const uint32_t K = (uint32_t)m.K;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    uint32_t bad = 0;
    long long scalar_from = 0;
    auto colour = [&](const uint32_t i) {
        const bool ok = i < K;
        bad += ok ? 0u : 1u;
        return pal[ok ? i : 0u];
    };
    if (VEC) {
        const long long n4 = n_px >> 2;
        for (long long g = gid; g < n4; g += stride) {
            uint32_t i0, i1, i2, i3;
            if (BYTES == 1) {
                const uint32_t v = static_cast<const uint32_t *>(index)[g];
                i0 = v & 0xFFu, i1 = (v >> 8) & 0xFFu, i2 = (v >> 16) & 0xFFu, i3 = v >> 24;
            } else {
                const uint2 v = static_cast<const uint2 *>(index)[g];
                i0 = v.x & 0xFFFFu, i1 = v.x >> 16, i2 = v.y & 0xFFFFu, i3 = v.y >> 16;
            }
            const uint32_t c0 = colour(i0), c1 = colour(i1), c2 = colour(i2), c3 = colour(i3);
            Word3 o;
            o.x = c0 | (c1 << 24);
            o.y = (c1 >> 8) | (c2 << 16);
            o.z = (c2 >> 16) | (c3 << 8);
            reinterpret_cast<Word3 *>(rgb)[g] = o;
        }
        scalar_from = n4 << 2;
    }
    for (long long i = scalar_from + gid; i < n_px; i += stride) {
        const uint32_t c = colour(load_index<BYTES>(index, i));
        uint8_t *p = rgb + 3 * i;
        p[0] = (uint8_t)c;
        p[1] = (uint8_t)(c >> 8);
        p[2] = (uint8_t)(c >> 16);
    }
    add_to_counter(n_bad, bad);
}

// Pillow's NEAREST coordinates (ImagingScaleAffine): xo_0 = 0.5 * scale, xo_{x+1} = xo_x + scale accumulated in double;
// thread 0 builds the column table, thread 1 the row table (as resize_tables_kernel of ordered.hip).
__global__ void plane_resize_tables_kernel(int *__restrict__ xtab, int *__restrict__ ytab, const int w, const int ow, const int h,
                                           const int oh)
{
    const int which = threadIdx.x;
    if (which > 1) return;
    const int n_in = which ? h : w, n_out = which ? oh : ow;
    int *tab = which ? ytab : xtab;
    const double a = (double)n_in / (double)n_out;
    double xo = __dmul_rn(a, 0.5);
    for (int x = 0; x < n_out; ++x) {
        const int v = (int)xo;
        tab[x] = v < n_in ? v : n_in - 1;
        xo = __dadd_rn(xo, a);
    }
}

template <typename T>
__global__ void plane_resize_kernel(const T *__restrict__ in, T *__restrict__ out, const int h, const int w, const int oh,
                                    const int ow, const int *__restrict__ xtab, const int *__restrict__ ytab)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const size_t f = blockIdx.z;
    if (x >= ow || y >= oh) return;
    out[f * oh * ow + (size_t)y * ow + x] = in[f * h * w + (size_t)ytab[y] * w + xtab[x]];
}

// The device view of a map; uploads it on first use.  `fn` names the caller in the error text.
int map_on_device(const dp_index_map *map, const char *fn, IndexMapDev &out)
{
    std::lock_guard<std::mutex> lock(map->mu);
    int dev = 0;
    DP_HIP(hipGetDevice(&dev));
    const IndexMapHost &h = map->host;
    if (!map->blob) {
        void *blob = nullptr;
        const size_t tab_bytes = sizeof(uint32_t) * (size_t)h.slots, col_bytes = sizeof(uint32_t) * (size_t)h.K;
        DP_HIP(hipMalloc(&blob, tab_bytes + col_bytes));
        hipError_t e = hipMemcpy(blob, h.table.data(), tab_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(static_cast<char *>(blob) + tab_bytes, h.colors.data(), col_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(blob);
            return hip_fail(e, "index map upload");
        }
        map->blob = blob;
        map->device = dev;
    } else if (map->device != dev) {
        set_error("%s: the index map lives on device %d, the current device is %d", fn, map->device, dev);
        return DP_EINVAL;
    }
    out.table = static_cast<const uint32_t *>(map->blob);
    out.colors = out.table + h.slots;
    out.K = h.K;
    out.slots = h.slots;
    out.rest_bits = h.rest_bits;
    out.max_probe = h.max_probe;
    out.mult = h.mult;
    return DP_OK;
}

inline unsigned grid_for(const long long work)
{
    const long long blocks = (work + kBlock - 1) / kBlock;
    return (unsigned)std::max<long long>(1, std::min<long long>(blocks, kMaxBlocks));
}

// the argument checks the two conversions share (`index` is whichever of a, b is the plane)
int check_conversion(const char *fn, const void *a, const void *b, const void *index, const long long n_px, const dp_index_map *map,
                     const int index_bytes, const void *counter)
{
    if (!a || !b || !map || !counter) {
        set_error("%s: NULL pointer", fn);
        return DP_EINVAL;
    }
    if (n_px < 0) {
        set_error("%s: n_px is negative", fn);
        return DP_EINVAL;
    }
    if (index_bytes != 1 && index_bytes != 2) {
        set_error("%s: index_bytes must be 1 or 2, not %d", fn, index_bytes);
        return DP_EINVAL;
    }
    if (index_bytes == 1 && map->host.K > 256) {
        set_error("%s: one-byte indices cannot hold a map of %d colours (index_bytes must be 2 above 256)", fn, map->host.K);
        return DP_EINVAL;
    }
    if (index_bytes == 2 && (reinterpret_cast<uintptr_t>(index) & 1u)) {
        set_error("%s: a two-byte index plane must be at an even address", fn);
        return DP_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(counter) & 7u) {
        set_error("%s: the counter must be 8-byte aligned", fn);
        return DP_EINVAL;
    }
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_index_map_create(const uint8_t *colors_host, int K, dp_index_map **out)
{
    if (!colors_host || !out) {
        set_error("dp_index_map_create: NULL pointer");
        return DP_EINVAL;
    }
    if (K < 1 || K > DP_MAX_COLORS) {
        set_error("dp_index_map_create: K must be in [1, %d], not %d", DP_MAX_COLORS, K);
        return DP_EINVAL;
    }
    dp_index_map *m = new dp_index_map();
    if (!index_map_build(colors_host, K, m->host)) {
        delete m;
        set_error("dp_index_map_create: no hash multiplier keeps every entry within %d slots of its home", kIndexMapMaxProbe);
        return DP_EUNSUPPORTED;
    }
    *out = m;
    return DP_OK;
}

void dp_index_map_destroy(dp_index_map *map)
{
    if (!map) return;
    if (map->blob) (void)hipFree(map->blob);
    delete map;
}

int dp_index_map_info(const dp_index_map *map, int *K, int *slots, int *max_probe)
{
    if (!map) {
        set_error("dp_index_map_info: NULL");
        return DP_EINVAL;
    }
    if (K) *K = map->host.K;
    if (slots) *slots = map->host.slots;
    if (max_probe) *max_probe = map->host.max_probe;
    return DP_OK;
}

int dp_index_from_rgb_u8(const uint8_t *rgb_dev, void *index_dev, int64_t n_px, const dp_index_map *map, int index_bytes,
                         int64_t *n_missing_dev, void *stream)
{
    const char *fn = "dp_index_from_rgb_u8";
    int rc = check_conversion(fn, rgb_dev, index_dev, index_dev, n_px, map, index_bytes, n_missing_dev);
    if (rc != DP_OK || n_px == 0) return rc;
    IndexMapDev m;
    rc = map_on_device(map, fn, m);
    if (rc != DP_OK) return rc;
    const bool vec = ((reinterpret_cast<uintptr_t>(rgb_dev) & 3u) | (reinterpret_cast<uintptr_t>(index_dev) & (4u * index_bytes - 1u))) == 0 &&
                     n_px >= 4;
    const unsigned grid = grid_for(vec ? n_px >> 2 : n_px);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(n_missing_dev);
    const long long n = n_px;
    if (index_bytes == 1) {
        if (vec)
            hipLaunchKernelGGL((index_from_rgb_kernel<1, true>), dim3(grid), dim3(kBlock), 0, s, rgb_dev, index_dev, n, m, cnt);
        else
            hipLaunchKernelGGL((index_from_rgb_kernel<1, false>), dim3(grid), dim3(kBlock), 0, s, rgb_dev, index_dev, n, m, cnt);
    } else {
        if (vec)
            hipLaunchKernelGGL((index_from_rgb_kernel<2, true>), dim3(grid), dim3(kBlock), 0, s, rgb_dev, index_dev, n, m, cnt);
        else
            hipLaunchKernelGGL((index_from_rgb_kernel<2, false>), dim3(grid), dim3(kBlock), 0, s, rgb_dev, index_dev, n, m, cnt);
    }
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int dp_rgb_from_index_u8(const void *index_dev, uint8_t *rgb_dev, int64_t n_px, const dp_index_map *map, int index_bytes,
                         int64_t *n_bad_dev, void *stream)
{
    const char *fn = "dp_rgb_from_index_u8";
    int rc = check_conversion(fn, index_dev, rgb_dev, index_dev, n_px, map, index_bytes, n_bad_dev);
    if (rc != DP_OK || n_px == 0) return rc;
    IndexMapDev m;
    rc = map_on_device(map, fn, m);
    if (rc != DP_OK) return rc;
    const bool vec = ((reinterpret_cast<uintptr_t>(rgb_dev) & 3u) | (reinterpret_cast<uintptr_t>(index_dev) & (4u * index_bytes - 1u))) == 0 &&
                     n_px >= 4;
    const unsigned grid = grid_for(vec ? n_px >> 2 : n_px);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(n_bad_dev);
    const long long n = n_px;
    if (index_bytes == 1) {
        if (vec)
            hipLaunchKernelGGL((rgb_from_index_kernel<1, true>), dim3(grid), dim3(kBlock), 0, s, index_dev, rgb_dev, n, m, cnt);
        else
            hipLaunchKernelGGL((rgb_from_index_kernel<1, false>), dim3(grid), dim3(kBlock), 0, s, index_dev, rgb_dev, n, m, cnt);
    } else {
        if (vec)
            hipLaunchKernelGGL((rgb_from_index_kernel<2, true>), dim3(grid), dim3(kBlock), 0, s, index_dev, rgb_dev, n, m, cnt);
        else
            hipLaunchKernelGGL((rgb_from_index_kernel<2, false>), dim3(grid), dim3(kBlock), 0, s, index_dev, rgb_dev, n, m, cnt);
    }
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int dp_resize_nearest_plane_u8(const void *in_dev, void *out_dev, int64_t n_frames, int h, int w, int oh, int ow, int elem_bytes,
                               void *stream)
{
    const char *fn = "dp_resize_nearest_plane_u8";
    if (!in_dev || !out_dev) {
        set_error("%s: NULL pointer", fn);
        return DP_EINVAL;
    }
    if (n_frames < 0 || h < 1 || w < 1 || oh < 1 || ow < 1) {
        set_error("%s: sizes must be >= 1 (n_frames >= 0)", fn);
        return DP_EINVAL;
    }
    if (elem_bytes != 1 && elem_bytes != 2) {
        set_error("%s: elem_bytes must be 1 or 2, not %d", fn, elem_bytes);
        return DP_EINVAL;
    }
    if (elem_bytes == 2 && ((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 1u)) {
        set_error("%s: a two-byte plane must be at an even address", fn);
        return DP_EINVAL;
    }
    if (oh > 65535 || n_frames > 65535) {
        set_error("%s: oh or n_frames > 65535 not supported", fn);
        return DP_EUNSUPPORTED;
    }
    if (n_frames == 0) return DP_OK;
    hipStream_t s = (hipStream_t)stream;
    int *tabs = nullptr;
    DP_HIP(hipMallocAsync((void **)&tabs, sizeof(int) * ((size_t)ow + oh), s));  // stream-ordered scratch
    hipLaunchKernelGGL(plane_resize_tables_kernel, dim3(1), dim3(64), 0, s, tabs, tabs + ow, w, ow, h, oh);
    const dim3 grid((ow + 255) / 256, oh, (unsigned)n_frames);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(plane_resize_kernel<uint8_t>, grid, dim3(256), 0, s, static_cast<const uint8_t *>(in_dev),
                           static_cast<uint8_t *>(out_dev), h, w, oh, ow, tabs, tabs + ow);
    else
        hipLaunchKernelGGL(plane_resize_kernel<uint16_t>, grid, dim3(256), 0, s, static_cast<const uint16_t *>(in_dev),
                           static_cast<uint16_t *>(out_dev), h, w, oh, ow, tabs, tabs + ow);
    hipError_t e = hipGetLastError();
    (void)hipFreeAsync(tabs, s);
    if (e != hipSuccess) return hip_fail(e, "plane resize launch");
    return DP_OK;
}

}  // extern "C"
