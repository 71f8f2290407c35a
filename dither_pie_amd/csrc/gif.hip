// Animated GIF output (include/ditherpie_hip_gif.h): inter-frame deltas of one-byte index planes and the LZW image data of
// every frame.  The stream is stated by host_logic.h: gif_lzw_encode; the kernels here write the same bytes.
//
// index_delta_kernel     grid (blocks per frame, frames): out = plane where it differs from the plane before, else the
//                        transparent index; four pixels per lane as one 4-byte load / store where the three bases of the
//                        frame are 4-byte aligned, one per lane otherwise and for the last n_px % 4 (the shape of
//                        index_from_rgb_kernel, indexed.hip).  Changed pixels are counted per lane, reduced per wave and
//                        added to the frame's counter once per wave that saw any.
// gif_lzw_chunk_kernel   one wave (a workgroup of 64) owns one chunk at a time, grid stride over the chunks of the batch.
//                        The dictionary is the 8192-slot open-addressing table of host_logic.h in LDS (32 KB, so 4 waves
//                        per CU beside their 256-byte pixel stage).  The match step is a dependent chain: every lane walks
//                        it with the same values (LDS reads of one address are broadcasts), so control flow is uniform by
//                        construction and nothing waits on another lane or wave; lane 0 alone stores.  Pixels arrive 256 at
//                        a time through LDS, the next block's loads in flight while the current one is matched.  The
//                        chunk's codes go to its workspace slot from bit 12 on: the 12 bits in front are left for the
//                        leading Clear, whose width only the chunk before knows.  The last chunk of a frame appends EOI.
//                        Loops: pixels <= chunk_px, a probe run <= 8192 slots, the table reset 128 steps.
// gif_lzw_layout_kernel  one wave per frame: the leading Clear of chunk j has the final width of chunk j - 1, so the length
//                        of chunk j's bits is that width + its body; an exclusive prefix (wave scan, 64 chunks a step)
//                        gives every chunk's bit offset in the frame, the Clear bit is set in the slot's reserved bits, the
//                        frame's bit total gives sizes[f].
// gif_lzw_pack_kernel    grid (blocks per frame, frames), one data byte per lane and step: a binary search for the chunk
//                        that holds the byte's first bit, then at most eight chunks contribute (a chunk has >= 3 bits...
//                        the loop takes at least one bit a step).  Byte i lands at 2 + i + i / 255; the lane of the first
//                        byte of a sub-block writes its length, lane 0 the min_code_size byte, the lane of the last byte
//                        the terminator.  Plain byte stores: no atomics, nothing read from `out`.
#include "dp_internal.h"

#include "../../include/ditherpie_hip_gif.h"

namespace dp {
namespace {

constexpr int kDeltaThreads = 256;
constexpr int kDeltaGroupsPerLane = 8;
constexpr int kDeltaMaxBlocksPerFrame = 256;
constexpr int kStagePx = 256;            // pixels a wave stages in LDS at a time (4 per lane)
constexpr int kChunkMaxBlocks = 256 * 4 * 4;   // 4 resident waves per CU, four rounds; the rest by grid stride
constexpr int kPackThreads = 256;
constexpr int kPackMaxBlocksPerFrame = 512;
constexpr int kReservedBits = 12;        // in front of a chunk's codes in its slot: room for the leading Clear

struct ChunkRec {
    unsigned long long off;   // bit offset of the chunk's leading Clear in the frame's stream
    uint32_t len;             // bits: leading Clear + body
    uint32_t start;           // bit of the slot at which the Clear begins (kReservedBits - its width)
};

__global__ __launch_bounds__(kDeltaThreads) void index_delta_kernel(const uint8_t *__restrict__ planes, const uint8_t *__restrict__ prev,
                                                                     const int has_prev, const uint32_t transparent, const long long n_px,
                                                                     uint8_t *__restrict__ out, unsigned long long *__restrict__ changed)
{
    const int f = (int)blockIdx.y;
    const uint8_t *__restrict__ cur = planes + (size_t)f * (size_t)n_px;
    const uint8_t *__restrict__ before = f > 0 ? cur - n_px : (has_prev ? prev : nullptr);   // (uniform over the workgroup)
    uint8_t *__restrict__ dst = out + (size_t)f * (size_t)n_px;
    const long long gid = (long long)blockIdx.x * kDeltaThreads + threadIdx.x, stride = (long long)gridDim.x * kDeltaThreads;
    uint32_t count = 0;
    long long scalar_from = 0;
    const bool vec = (((uintptr_t)cur | (uintptr_t)dst | (uintptr_t)(before ? before : cur)) & 3u) == 0;
    if (vec) {
        const long long n4 = n_px >> 2;
        const uint32_t t4 = transparent * 0x01010101u;
        for (long long g = gid; g < n4; g += stride) {
            const uint32_t a = reinterpret_cast<const uint32_t *>(cur)[g];
            uint32_t r = a;
            if (before) {
                const uint32_t x = a ^ reinterpret_cast<const uint32_t *>(before)[g];
                uint32_t same = 0;   // 0xFF in every byte that is equal
                same |= (x & 0x000000FFu) ? 0u : 0x000000FFu;
                same |= (x & 0x0000FF00u) ? 0u : 0x0000FF00u;
                same |= (x & 0x00FF0000u) ? 0u : 0x00FF0000u;
                same |= (x & 0xFF000000u) ? 0u : 0xFF000000u;
                r = (a & ~same) | (t4 & same);
                count += 4u - (uint32_t)__popc(same) / 8u;
            }
            reinterpret_cast<uint32_t *>(dst)[g] = r;
        }
        scalar_from = n4 << 2;
    }
    for (long long i = scalar_from + gid; i < n_px; i += stride) {
        const uint8_t a = cur[i];
        const bool same = before && before[i] == a;
        dst[i] = same ? (uint8_t)transparent : a;
        count += (before && !same) ? 1u : 0u;
    }
    if (!before) {   // a first frame without a plane before it goes out whole: every pixel counts
        if (gid == 0) atomicAdd(&changed[f], (unsigned long long)n_px);
        return;
    }
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off);
    if ((threadIdx.x & 63u) == 0 && count) atomicAdd(&changed[f], (unsigned long long)count);
}

__global__ __launch_bounds__(64) void gif_lzw_chunk_kernel(const uint8_t *__restrict__ planes, const long long n_px, const long long chunk_px,
                                                           const int n_chunks, const int total_chunks, const int mcs,
                                                           uint8_t *__restrict__ slots, const long long slot_bytes, uint2 *__restrict__ meta)
{
    __shared__ uint32_t tab[kGifSlots];
    __shared__ uint32_t s_px[kStagePx / 4];
    const int lane = (int)threadIdx.x;
    const uint32_t clear = 1u << mcs, mask = clear - 1u;
    const int slot_words = (int)(slot_bytes >> 2);
    for (int id = (int)blockIdx.x; id < total_chunks; id += (int)gridDim.x) {
        const int f = id / n_chunks, j = id - f * n_chunks;
        const long long at = (long long)j * chunk_px;
        const long long n = chunk_px < n_px - at ? chunk_px : n_px - at;
        const uint8_t *__restrict__ px = planes + (size_t)f * (size_t)n_px + (size_t)at;
        uint32_t *__restrict__ slot = reinterpret_cast<uint32_t *>(slots + (size_t)id * (size_t)slot_bytes);

        auto load4 = [&](const long long base) {   // pixels base + 4 lane ... + 3 of the chunk, 0 beyond its end
            uint32_t v = 0;
            const long long p = base + 4 * lane;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p + k < n) v |= (uint32_t)px[p + k] << (8 * k);
            return v;
        };

        __syncthreads();   // (the chunk before is done with both arrays)
        for (int i = lane; i < kGifSlots; i += 64) tab[i] = kGifEmpty;
        s_px[lane] = load4(0);
        __syncthreads();

        unsigned long long acc = 0;
        int nbits = kReservedBits, wi = 0;
        auto put = [&](const uint32_t code, const int width) {
            acc |= (unsigned long long)code << nbits;
            nbits += width;
            if (nbits >= 32) {
                if (lane == 0 && wi < slot_words) slot[wi] = (uint32_t)acc;
                ++wi;
                acc >>= 32;
                nbits -= 32;
            }
        };

        int width = mcs + 1;
        uint32_t next = clear + 2u;
        uint32_t cur = s_px[0] & mask;
        for (long long base = 0; base < n; base += kStagePx) {
            const uint32_t ahead = load4(base + kStagePx);   // in flight while this block is matched
            const int first = base == 0 ? 1 : 0;
            const int count = (int)(n - base < kStagePx ? n - base : kStagePx);
            for (int i = first; i < count; ++i) {
                const uint32_t c = (s_px[i >> 2] >> (8 * (i & 3))) & mask;
                const uint32_t key = (cur << 8) | c;
                uint32_t at_slot = (key * 0x9E3779B1u) >> 19, found = kGifEmpty;
                for (int probe = 0; probe < kGifSlots; ++probe) {
                    const uint32_t e = tab[at_slot];
                    if (e == kGifEmpty) break;
                    if ((e >> 12) == key) {
                        found = e & 0xFFFu;
                        break;
                    }
                    at_slot = (at_slot + 1u) & (uint32_t)(kGifSlots - 1);
                }
                if (found != kGifEmpty) {
                    cur = found;
                    continue;
                }
                put(cur, width);
                if (next < 4096u) {
                    if (lane == 0) tab[at_slot] = (key << 12) | next;
                    if (next == (1u << width) && width < 12) ++width;
                    ++next;
                } else {
                    put(clear, 12);
                    width = mcs + 1;
                    next = clear + 2u;
                    __syncthreads();
                    for (int k = lane; k < kGifSlots; k += 64) tab[k] = kGifEmpty;
                    __syncthreads();
                }
                cur = c;
            }
            __syncthreads();
            s_px[lane] = ahead;
            __syncthreads();
        }
        put(cur, width);
        if (next < 4096u && next == (1u << width) && width < 12) ++width;   // the decoder's lagging entry
        if (j == n_chunks - 1) put(clear + 1u, width);                       // EOI closes the frame
        if (nbits > 0 && lane == 0 && wi < slot_words) slot[wi] = (uint32_t)acc;
        if (lane == 0) meta[id] = make_uint2((uint32_t)(32 * wi + nbits - kReservedBits), (uint32_t)width);
    }
}

__global__ __launch_bounds__(64) void gif_lzw_layout_kernel(const uint2 *__restrict__ meta, const int n_chunks, const int mcs,
                                                            uint8_t *__restrict__ slots, const long long slot_bytes, ChunkRec *__restrict__ rec,
                                                            unsigned long long *__restrict__ frame_bits, long long *__restrict__ sizes)
{
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const size_t row = (size_t)f * (size_t)n_chunks;
    unsigned long long carry = 0;
    for (int base = 0; base < n_chunks; base += 64) {
        const int j = base + lane;
        const bool valid = j < n_chunks;
        uint32_t body = 0, cw = 0;
        if (valid) {
            body = meta[row + j].x;
            cw = j == 0 ? (uint32_t)(mcs + 1) : meta[row + j - 1].y;   // the width in force at the end of the chunk before
        }
        const unsigned long long len = valid ? (unsigned long long)(cw + body) : 0ull;
        unsigned long long incl = len;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (valid) {
            ChunkRec r;
            r.off = carry + incl - len;
            r.len = (uint32_t)len;
            r.start = (uint32_t)kReservedBits - cw;
            rec[row + j] = r;
            uint32_t *word0 = reinterpret_cast<uint32_t *>(slots + (row + j) * (size_t)slot_bytes);
            *word0 |= 1u << (r.start + (uint32_t)mcs);   // the Clear code: bit min_code_size of its cw bits
        }
        carry += __shfl(incl, 63);
    }
    if (lane == 0) {
        frame_bits[f] = carry;
        const unsigned long long d = (carry + 7ull) >> 3;
        sizes[f] = (long long)(1ull + d + (d + 254ull) / 255ull + 1ull);
    }
}

__global__ __launch_bounds__(kPackThreads) void gif_lzw_pack_kernel(const ChunkRec *__restrict__ rec, const unsigned long long *__restrict__ frame_bits,
                                                                     const uint8_t *__restrict__ slots, const long long slot_bytes, const int n_chunks,
                                                                     const int mcs, uint8_t *__restrict__ out, const long long out_stride)
{
    const int f = (int)blockIdx.y;
    const size_t row = (size_t)f * (size_t)n_chunks;
    const ChunkRec *__restrict__ R = rec + row;
    const unsigned long long bits = frame_bits[f], d = (bits + 7ull) >> 3;
    uint8_t *__restrict__ dst = out + (size_t)f * (size_t)out_stride;
    const unsigned long long limit = (unsigned long long)out_stride;   // (the bound keeps every index below it; checked all the same)
    const unsigned long long gid = (unsigned long long)blockIdx.x * kPackThreads + threadIdx.x, stride = (unsigned long long)gridDim.x * kPackThreads;
    for (unsigned long long i = gid; i < d; i += stride) {
        unsigned long long pos = 8ull * i;
        const unsigned long long end = pos + 8ull < bits ? pos + 8ull : bits;
        int lo = 0, hi = n_chunks - 1;
        for (int step = 0; step < 32 && lo < hi; ++step) {   // the last chunk whose first bit is at or before pos
            const int mid = lo + (hi - lo + 1) / 2;
            if (R[mid].off <= pos) lo = mid;
            else hi = mid - 1;
        }
        uint32_t byte = 0;
        int j = lo;
        for (int step = 0; step < 8 && pos < end && j < n_chunks; ++step) {
            const ChunkRec r = R[j];
            const unsigned long long rel = pos - r.off;
            const unsigned long long avail = (unsigned long long)r.len - rel;
            const unsigned long long want = end - pos;
            const uint32_t take = (uint32_t)(avail < want ? avail : want);
            const unsigned long long sb = (unsigned long long)r.start + rel;
            const uint8_t *__restrict__ s = slots + (row + (size_t)j) * (size_t)slot_bytes + (size_t)(sb >> 3);   // (s[1]: the slot's padding at most)
            const uint32_t v = ((uint32_t)s[0] | ((uint32_t)s[1] << 8)) >> (uint32_t)(sb & 7ull);
            byte |= (v & ((1u << take) - 1u)) << (uint32_t)(pos - 8ull * i);
            pos += take;
            if (avail <= want) ++j;
        }
        const unsigned long long blk = i / 255ull, where = 2ull + i + blk;
        if (where < limit) dst[where] = (uint8_t)byte;
        if (i == blk * 255ull) {   // the first byte of a sub-block: its length goes in front
            const unsigned long long left = d - i;
            if (where - 1ull < limit) dst[where - 1ull] = (uint8_t)(left < 255ull ? left : 255ull);
        }
        if (i == 0) dst[0] = (uint8_t)mcs;
        if (i == d - 1ull && where + 1ull < limit) dst[where + 1ull] = 0;
    }
}

struct LzwPlan {
    long long n_px, chunk_px, slot_bytes;
    int n_chunks;
    long long total_chunks;
    size_t rec_off, meta_off, bits_off, slots_off, total;
};

size_t round16(const size_t v) { return (v + 15u) & ~(size_t)15u; }

// n_frames >= 0, h, w >= 1, h * w < 2^31, chunk_px >= 1 (the callers check)
LzwPlan lzw_plan(const int n_frames, const int h, const int w, const int64_t chunk_px)
{
    LzwPlan p;
    p.n_px = (long long)h * (long long)w;
    p.chunk_px = chunk_px < p.n_px ? chunk_px : p.n_px;
    p.n_chunks = (int)gif_chunks(p.n_px, p.chunk_px);
    p.total_chunks = (long long)p.n_chunks * (long long)n_frames;
    // a slot: the reserved bits, a code per pixel, the Clears inside the chunk, EOI and one to spare, 12 bits each, in whole
    // words, and a word of padding (the pack kernel reads one byte past a chunk's last)
    const long long codes = p.chunk_px + p.chunk_px / kGifCodesPerClear + 2;
    p.slot_bytes = 4 * ((kReservedBits + 12 * codes + 31) / 32) + 4;
    p.rec_off = 0;
    p.meta_off = round16((size_t)p.total_chunks * sizeof(ChunkRec));
    p.bits_off = p.meta_off + round16((size_t)p.total_chunks * sizeof(uint2));
    p.slots_off = p.bits_off + round16((size_t)n_frames * sizeof(unsigned long long));
    p.total = p.slots_off + (size_t)p.total_chunks * (size_t)p.slot_bytes;
    return p;
}

bool lzw_geometry_ok(const int h, const int w, const int64_t chunk_px)
{
    return h >= 1 && w >= 1 && (long long)h * (long long)w < (1LL << 31) && chunk_px >= 1;
}

int launch_index_delta(const uint8_t *planes, int n_frames, long long n_px, uint8_t *prev, int has_prev, int transparent, uint8_t *out,
                       unsigned long long *changed, hipStream_t s)
{
    DP_HIP(hipMemsetAsync(changed, 0, (size_t)n_frames * sizeof(unsigned long long), s));
    const long long groups = (n_px + 3) / 4, per_block = (long long)kDeltaThreads * kDeltaGroupsPerLane;
    long long bpf = (groups + per_block - 1) / per_block;
    bpf = bpf < 1 ? 1 : (bpf > kDeltaMaxBlocksPerFrame ? kDeltaMaxBlocksPerFrame : bpf);
    hipLaunchKernelGGL(index_delta_kernel, dim3((unsigned)bpf, (unsigned)n_frames), dim3(kDeltaThreads), 0, s, planes, (const uint8_t *)prev, has_prev,
                       (uint32_t)transparent, n_px, out, changed);
    DP_HIP(hipGetLastError());
    DP_HIP(hipMemcpyAsync(prev, planes + (size_t)(n_frames - 1) * (size_t)n_px, (size_t)n_px, hipMemcpyDeviceToDevice, s));
    return DP_OK;
}

int launch_gif_lzw(const uint8_t *planes, int n_frames, int mcs, const LzwPlan &p, uint8_t *out, long long out_stride, long long *sizes, uint8_t *ws,
                   hipStream_t s)
{
    ChunkRec *rec = reinterpret_cast<ChunkRec *>(ws + p.rec_off);
    uint2 *meta = reinterpret_cast<uint2 *>(ws + p.meta_off);
    unsigned long long *frame_bits = reinterpret_cast<unsigned long long *>(ws + p.bits_off);
    uint8_t *slots = ws + p.slots_off;
    const int total = (int)p.total_chunks;
    const int grid = total < kChunkMaxBlocks ? total : kChunkMaxBlocks;
    hipLaunchKernelGGL(gif_lzw_chunk_kernel, dim3((unsigned)grid), dim3(64), 0, s, planes, p.n_px, p.chunk_px, p.n_chunks, total, mcs, slots, p.slot_bytes,
                       meta);
    DP_HIP(hipGetLastError());
    hipLaunchKernelGGL(gif_lzw_layout_kernel, dim3((unsigned)n_frames), dim3(64), 0, s, (const uint2 *)meta, p.n_chunks, mcs, slots, p.slot_bytes, rec,
                       frame_bits, sizes);
    DP_HIP(hipGetLastError());
    const long long bound_d = (long long)gif_lzw_bound(p.n_px, p.chunk_px);
    long long bpf = (bound_d / 4 + kPackThreads - 1) / kPackThreads;   // dithered content compresses: a quarter of the bound per pass
    bpf = bpf < 1 ? 1 : (bpf > kPackMaxBlocksPerFrame ? kPackMaxBlocksPerFrame : bpf);
    hipLaunchKernelGGL(gif_lzw_pack_kernel, dim3((unsigned)bpf, (unsigned)n_frames), dim3(kPackThreads), 0, s, (const ChunkRec *)rec,
                       (const unsigned long long *)frame_bits, (const uint8_t *)slots, p.slot_bytes, p.n_chunks, mcs, out, out_stride);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

bool overlap(const void *a, const size_t na, const void *b, const size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_index_delta_u8(const uint8_t *planes_dev, int n_frames, int64_t n_px, uint8_t *prev_plane_dev, int has_prev, int transparent,
                      uint8_t *out_dev, int64_t *changed_dev, void *stream)
{
    if (!planes_dev || !prev_plane_dev || !out_dev || !changed_dev || ((uintptr_t)changed_dev & 7) || n_px < 1 || n_frames < 0 || transparent < 0 ||
        transparent > 255) {
        set_error("dp_index_delta_u8: bad argument (n_px >= 1, n_frames >= 0, transparent in 0 ... 255, changed_dev 8-byte aligned)");
        return DP_EINVAL;
    }
    if (n_frames > 65535) {
        set_error("dp_index_delta_u8: at most 65535 frames per call, not %d", n_frames);
        return DP_EUNSUPPORTED;
    }
    const size_t all = (size_t)(n_frames > 0 ? n_frames : 1) * (size_t)n_px;
    if (overlap(out_dev, all, planes_dev, all) || overlap(out_dev, all, prev_plane_dev, (size_t)n_px) ||
        overlap(prev_plane_dev, (size_t)n_px, planes_dev, all)) {
        set_error("dp_index_delta_u8: bad argument (out_dev, planes_dev and prev_plane_dev must not overlap: no in-place operation)");
        return DP_EINVAL;
    }
    if (n_frames == 0) return DP_OK;
    return launch_index_delta(planes_dev, n_frames, (long long)n_px, prev_plane_dev, has_prev ? 1 : 0, transparent, out_dev,
                              reinterpret_cast<unsigned long long *>(changed_dev), (hipStream_t)stream);
}

size_t dp_gif_lzw_bound_bytes(int h, int w, int64_t chunk_px)
{
    if (!lzw_geometry_ok(h, w, chunk_px)) return 0;
    return (size_t)gif_lzw_bound((int64_t)h * (int64_t)w, chunk_px);
}

size_t dp_gif_lzw_workspace_bytes(int n_frames, int h, int w, int64_t chunk_px)
{
    if (!lzw_geometry_ok(h, w, chunk_px) || n_frames < 0) return 0;
    return lzw_plan(n_frames, h, w, chunk_px).total;
}

static int check_lzw(const char *fn, const void *planes, int n_frames, int h, int w, int min_code_size, int64_t chunk_px, const void *out,
                     int64_t out_stride, const void *sizes)
{
    if (!planes || !out || !sizes || n_frames < 0 || !lzw_geometry_ok(h, w, chunk_px) || min_code_size < 2 || min_code_size > 8) {
        set_error("%s: bad argument (h, w >= 1, h * w < 2^31, n_frames >= 0, min_code_size in 2 ... 8, chunk_px >= 1)", fn);
        return DP_EINVAL;
    }
    const uint64_t need = gif_lzw_bound((int64_t)h * (int64_t)w, chunk_px);
    if (out_stride < 0 || (uint64_t)out_stride < need) {
        set_error("%s: bad argument (out_stride of %lld bytes is below the bound of %llu for %d x %d at chunk_px %lld)", fn, (long long)out_stride,
                  (unsigned long long)need, h, w, (long long)chunk_px);
        return DP_EINVAL;
    }
    return DP_OK;
}

int dp_gif_lzw_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int min_code_size, int64_t chunk_px, uint8_t *out_dev,
                         int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream)
{
    const char *fn = "dp_gif_lzw_encode_u8";
    const int rc = check_lzw(fn, planes_dev, n_frames, h, w, min_code_size, chunk_px, out_dev, out_stride, sizes_dev);
    if (rc != DP_OK) return rc;
    if (!ws_dev || ((uintptr_t)ws_dev & 15) || ((uintptr_t)sizes_dev & 7)) {
        set_error("%s: bad argument (ws_dev 16-byte, sizes_dev 8-byte aligned)", fn);
        return DP_EINVAL;
    }
    if (n_frames > 65535) {
        set_error("%s: at most 65535 frames per call, not %d", fn, n_frames);
        return DP_EUNSUPPORTED;
    }
    const LzwPlan p = lzw_plan(n_frames, h, w, chunk_px);
    if (p.total_chunks >= (1LL << 31)) {
        set_error("%s: %d frames of %d chunks are 2^31 chunks or more: cut the batch or raise chunk_px", fn, n_frames, p.n_chunks);
        return DP_EUNSUPPORTED;
    }
    if (ws_bytes < p.total) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, p.total);
        return DP_EWORKSPACE;
    }
    if (n_frames == 0) return DP_OK;
    return launch_gif_lzw(planes_dev, n_frames, min_code_size, p, out_dev, (long long)out_stride, reinterpret_cast<long long *>(sizes_dev),
                          static_cast<uint8_t *>(ws_dev), (hipStream_t)stream);
}

int dp_gif_lzw_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int min_code_size, int64_t chunk_px, uint8_t *out_host,
                       int64_t out_stride, int64_t *sizes_host)
{
    const int rc = check_lzw("dp_gif_lzw_host_u8", planes_host, n_frames, h, w, min_code_size, chunk_px, out_host, out_stride, sizes_host);
    if (rc != DP_OK) return rc;
    try {
        const int64_t n_px = (int64_t)h * (int64_t)w;
        std::vector<uint8_t> frame;
        for (int f = 0; f < n_frames; ++f) {
            gif_lzw_encode(planes_host + (size_t)f * (size_t)n_px, n_px, min_code_size, chunk_px, frame);
            if ((int64_t)frame.size() > out_stride) {   // (the bound says it cannot be)
                set_error("dp_gif_lzw_host_u8: frame %d of %zu bytes exceeds the stride", f, frame.size());
                return DP_EINVAL;
            }
            std::copy(frame.begin(), frame.end(), out_host + (size_t)f * (size_t)out_stride);
            sizes_host[f] = (int64_t)frame.size();
        }
    } catch (const std::exception &e) {
        set_error("dp_gif_lzw_host_u8: %s", e.what());
        return DP_ENOMEM;
    }
    return DP_OK;
}

}  // extern "C"
