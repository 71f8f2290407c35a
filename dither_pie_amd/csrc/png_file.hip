// Finished PNG chunks on the device (include/ditherpie_hip_png_file.h): CRC-32 of byte runs and the IDAT / fdAT chunks around
// the streams of png.hip, packed back to back.  The statements are host_logic.h: crc32_update, png_file_assemble.
//
// CRC.  A register run from zero ("pure", host_logic.h) is linear and blind to leading zeros, so a run is cut from its END:
//   crc_parts_kernel   one workgroup step covers kCrcSpanBytes that end g spans before the last 4-byte boundary of the run's
//                      addresses.  The span is staged in LDS with aligned dword loads (bytes in front of the run are zeros;
//                      the one word the run's first byte may share with them is read byte by byte), lane t runs the
//                      register over the 16 words of piece t (slicing by four, tables in LDS), lifts the result by
//                      x^(8 * 64 * (255 - t)) with one multiplication modulo the polynomial, and the 256 results are
//                      xor-ed: one partial word per span.
//   crc_join           one wave: lane l lifts partial g = l, l + 64, ... by x^(8 * 16384 * g) (squares from a table) and the
//                      wave xor-s them; lane 0 feeds the up to three bytes behind the boundary, adds the register of
//                      whatever stood in front of the run (0xFFFFFFFF, or the chunk type and sequence number) lifted by
//                      the run's length, and inverts.
// LDS (cdna_hip_programming.md 2: ds_read_b32 banks are dword % 32, conflicts per 32-lane half): a piece is 16 dwords, so
// piece t would start on bank 16 t % 32 -- 16 lanes on each of two banks.  The staging skips one dword after every 16
// (data word k lives at k + k / 16): piece t starts at 17 t and the 32 lanes of a half read 32 different banks.  The table
// lookups are indexed by data and conflict as chance has it; four lookups per dword are independent of each other.
//
// Chunks.  file_layout_kernel (one workgroup) turns the clamped sizes into the frame boundaries; file_copy_kernel writes
// every frame's bytes one aligned destination dword per lane: a dword that lies inside the stream is put together from two
// aligned source dwords (v_alignbyte), everything else -- the prefix, the length, type and sequence number, the suffix, and
// the dwords a frame shares with its neighbours -- byte by byte.  Wave 0 of a frame's first workgroup joins the CRC.
#include "dp_internal.h"

#include "../../include/ditherpie_hip_png_file.h"

namespace dp {
namespace {

static_assert(kCrcPieceBytes == DP_PNG_CRC_PIECE_BYTES && kCrcSpanBytes == DP_PNG_CRC_SPAN_BYTES, "the header states the constants of host_logic.h");

__constant__ const CrcTables d_crc = make_crc_tables();

constexpr int kCrcThreads = kCrcPieces;                       // one lane per piece
constexpr int kCrcPieceWords = kCrcPieceBytes / 4;            // 16
constexpr int kCrcSpanWords = kCrcSpanBytes / 4;
constexpr int kCrcLdsWords = kCrcSpanWords + kCrcSpanWords / 16;
constexpr int kCrcMaxBlocksPerRun = 1024;                     // more spans than that are taken by grid stride
constexpr int kCopyThreads = 256;
constexpr int kCopyWordsPerBlock = kCopyThreads * 16;         // what sizes the grid; the loop is a grid stride
constexpr int kCopyMaxBlocksPerFrame = 512;
constexpr int kLayoutThreads = 256;

static_assert(kCrcPieceWords == 16 && kCrcThreads % 64 == 0, "the LDS skew assumes 16-dword pieces");

// where a run's pieces are: offsets relative to its first byte
struct RunCut {
    int64_t n;        // clamped size
    int64_t e4;       // offset of the last 4-byte boundary of its addresses, when that lies behind the first byte; else 0
    int n_parts;      // spans in front of e4
};

__device__ __forceinline__ RunCut cut_run(const uint8_t *base, const int64_t size, const int64_t stride)
{
    RunCut c;
    c.n = png_file_clamp(size, stride);
    const int64_t tail = (int64_t)(((uintptr_t)base + (uintptr_t)c.n) & 3u);
    c.e4 = c.n > tail ? c.n - tail : 0;
    c.n_parts = (int)((c.e4 + kCrcSpanBytes - 1) / kCrcSpanBytes);
    return c;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// parts[run * parts_stride + g]: the pure register of the span that ends g spans before e4
__global__ __launch_bounds__(kCrcThreads) void crc_parts_kernel(const uint8_t *__restrict__ data, const int64_t stride, const long long *__restrict__ sizes,
                                                                uint32_t *__restrict__ parts, const int64_t parts_stride)
{
    __shared__ uint32_t tab[4 * 256];
    __shared__ uint32_t span[kCrcLdsWords];
    __shared__ uint32_t red[kCrcThreads / 64];
    const int t = (int)threadIdx.x;
    const int run = (int)blockIdx.y;
    const uint8_t *base = data + (int64_t)run * stride;
    const RunCut c = cut_run(base, (int64_t)sizes[run], stride);
    if ((int)blockIdx.x >= c.n_parts) return;                 // (uniform over the workgroup)
    for (int i = t; i < 4 * 256; i += kCrcThreads) tab[i] = d_crc.byte[i >> 8][i & 255];
    const uint32_t lift = d_crc.piece[kCrcPieces - 1 - t];
    for (int g = (int)blockIdx.x; g < c.n_parts; g += (int)gridDim.x) {
        const int64_t lo = c.e4 - (int64_t)(g + 1) * kCrcSpanBytes;   // may lie in front of the run: zeros there
#pragma unroll 4
        for (int k = t; k < kCrcSpanWords; k += kCrcThreads) {
            const int64_t o = lo + 4 * (int64_t)k;            // base + o is 4-byte aligned, o + 4 <= e4 <= n
            uint32_t v = 0;
            if (o >= 0) {
                v = *reinterpret_cast<const uint32_t *>(base + o);
            } else if (o > -4) {
                for (int b = (int)-o; b < 4; ++b) v |= (uint32_t)base[o + b] << (8 * b);
            }
            span[k + (k >> 4)] = v;
        }
        __syncthreads();
        uint32_t r = 0;
        const uint32_t *mine = span + 17 * t;
#pragma unroll
        for (int j = 0; j < kCrcPieceWords; ++j) {
            r ^= mine[j];
            r = tab[768 + (r & 255u)] ^ tab[512 + ((r >> 8) & 255u)] ^ tab[256 + ((r >> 16) & 255u)] ^ tab[r >> 24];
        }
        r = wave_xor(crc_gfmul(r, lift));
        if ((t & 63) == 0) red[t >> 6] = r;
        __syncthreads();                                       // red is complete, and nobody reads `span` any more
        if (t == 0) {
            uint32_t all = 0;
            for (int i = 0; i < kCrcThreads / 64; ++i) all ^= red[i];
            parts[(int64_t)run * parts_stride + g] = all;
        }
    }
}

// One wave, every lane calls it; the result is valid in lane 0: ~(state0 x^(8 n) + pure(run))
__device__ __forceinline__ uint32_t crc_join(const uint8_t *base, const RunCut &c, const uint32_t *__restrict__ parts, const uint32_t state0, const int lane)
{
    uint32_t acc = 0;
    for (int g = lane; g < c.n_parts; g += 64) acc ^= crc_shift_bytes(parts[g], (uint64_t)g * (uint64_t)kCrcSpanBytes, d_crc.x8);
    acc = wave_xor(acc);
    if (lane != 0) return 0;
    for (int64_t o = c.e4; o < c.n; ++o) acc = crc_bits8(acc ^ (uint32_t)base[o]);
    return ~(crc_shift_bytes(state0, (uint64_t)c.n, d_crc.x8) ^ acc);
}

__global__ __launch_bounds__(64) void crc_join_kernel(const uint8_t *__restrict__ data, const int64_t stride, const long long *__restrict__ sizes,
                                                      const uint32_t *__restrict__ parts, const int64_t parts_stride, uint32_t *__restrict__ crc)
{
    const int run = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint8_t *base = data + (int64_t)run * stride;
    const RunCut c = cut_run(base, (int64_t)sizes[run], stride);
    const uint32_t v = crc_join(base, c, parts + (int64_t)run * parts_stride, 0xFFFFFFFFu, lane);
    if (lane == 0) crc[run] = v;
}

struct FileArgs {
    const uint8_t *streams;
    int64_t stream_stride;
    const long long *sizes;
    int n_frames, n_idat;
    uint32_t seq0, seq_step;
    const uint8_t *pre;
    int64_t pre_stride;
    int pre_bytes;
    const uint8_t *post;
    int post_bytes;
    uint8_t *out;
    long long *offsets;
};

__device__ __forceinline__ int64_t frame_bytes(const FileArgs &a, const int f)
{
    return (int64_t)a.pre_bytes + (f >= a.n_idat ? 12 : 8) + png_file_clamp((int64_t)a.sizes[f], a.stream_stride) + 4 + (int64_t)a.post_bytes;
}

// offsets[0 ... n_frames]: lane t sums its stretch of frames, lane 0 turns the 256 sums into starts, every lane writes its own
__global__ __launch_bounds__(kLayoutThreads) void file_layout_kernel(const FileArgs a)
{
    __shared__ long long start[kLayoutThreads];
    const int t = (int)threadIdx.x;
    const int per = (a.n_frames + kLayoutThreads - 1) / kLayoutThreads;
    const int f0 = t * per < a.n_frames ? t * per : a.n_frames, f1 = f0 + per < a.n_frames ? f0 + per : a.n_frames;
    long long sum = 0;
    for (int f = f0; f < f1; ++f) sum += frame_bytes(a, f);
    start[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long at = 0;
        for (int i = 0; i < kLayoutThreads; ++i) {
            const long long s = start[i];
            start[i] = at;
            at += s;
        }
        a.offsets[a.n_frames] = at;
    }
    __syncthreads();
    long long at = start[t];
    for (int f = f0; f < f1; ++f) {
        a.offsets[f] = at;
        at += frame_bytes(a, f);
    }
}

__global__ __launch_bounds__(kCopyThreads) void file_copy_kernel(const FileArgs a, const uint32_t *__restrict__ parts, const int64_t parts_stride)
{
    const int f = (int)blockIdx.y, t = (int)threadIdx.x;
    const bool fdat = f >= a.n_idat;
    const uint8_t *src = a.streams + (int64_t)f * a.stream_stride;
    const int64_t n = png_file_clamp((int64_t)a.sizes[f], a.stream_stride);
    const int hdr = fdat ? 12 : 8;
    const uint32_t seq = a.seq0 + (uint32_t)(f - a.n_idat) * a.seq_step;
    // the frame's bytes by position: [0, p1) prefix, [p1, p2) length, type, sequence number, [p2, p3) stream, [p3, p4) CRC,
    // [p4, total) suffix
    const int64_t p1 = a.pre_bytes, p2 = p1 + hdr, p3 = p2 + n, p4 = p3 + 4, total = p4 + a.post_bytes;
    uint8_t *dst = a.out + (int64_t)a.offsets[f];

    if (blockIdx.x == 0 && t < 64) {
        uint32_t state = 0xFFFFFFFFu;
        if (t == 0) {
            const uint32_t type = png_file_type(fdat);
            for (int i = 3; i >= 0; --i) state = crc_bits8(state ^ ((type >> (8 * i)) & 255u));
            if (fdat)
                for (int i = 3; i >= 0; --i) state = crc_bits8(state ^ ((seq >> (8 * i)) & 255u));
        }
        const uint32_t crc = crc_join(src, cut_run(src, n, a.stream_stride), parts + (int64_t)f * parts_stride, state, t);
        if (t == 0)
            for (int i = 0; i < 4; ++i) dst[p3 + i] = (uint8_t)(crc >> (24 - 8 * i));
    }

    const uintptr_t d0 = (uintptr_t)dst;
    const int64_t w0 = (int64_t)(d0 >> 2), n_words = (int64_t)((d0 + (uintptr_t)total + 3u) >> 2) - w0;   // aligned dwords the frame touches
    const uintptr_t s_lo = ((uintptr_t)src + 3u) & ~(uintptr_t)3u, s_hi = ((uintptr_t)src + (uintptr_t)n) & ~(uintptr_t)3u;   // whole dwords of the stream
    for (int64_t wi = (int64_t)blockIdx.x * kCopyThreads + t; wi < n_words; wi += (int64_t)gridDim.x * kCopyThreads) {
        const int64_t k = (int64_t)(((uintptr_t)(w0 + wi) << 2) - d0);   // position of the dword's first byte: -3 ... total - 1
        if (k >= p2 && k + 4 <= p3) {
            const uintptr_t s = (uintptr_t)src + (uintptr_t)(k - p2);
            const uintptr_t sa = s & ~(uintptr_t)3u;
            const unsigned sh = (unsigned)(s & 3u);
            if (sa >= s_lo && sa + (sh ? 8u : 4u) <= s_hi) {
                const uint32_t lo = *reinterpret_cast<const uint32_t *>(sa);
                const uint32_t v = sh ? __builtin_amdgcn_alignbyte(*reinterpret_cast<const uint32_t *>(sa + 4), lo, sh) : lo;
                *reinterpret_cast<uint32_t *>(dst + k) = v;
                continue;
            }
        }
        for (int b = 0; b < 4; ++b) {
            const int64_t p = k + b;
            if (p < 0 || p >= total || (p >= p3 && p < p4)) continue;   // a neighbour's byte, or the CRC (wave 0 above)
            uint8_t v;
            if (p < p1) {
                v = a.pre[(int64_t)f * a.pre_stride + p];
            } else if (p < p2) {
                const int j = (int)(p - p1);
                const uint32_t word = j < 4 ? (uint32_t)n + (fdat ? 4u : 0u) : j < 8 ? png_file_type(fdat) : seq;
                v = (uint8_t)(word >> (24 - 8 * (j & 3)));
            } else if (p < p3) {
                v = src[p - p2];
            } else {
                v = a.post[p - p4];
            }
            dst[p] = v;
        }
    }
}

size_t round16(const size_t v) { return (v + 15u) & ~(size_t)15u; }
int64_t parts_per_run(const int64_t stride) { return stride > kCrcSpanBytes ? (stride + kCrcSpanBytes - 1) / kCrcSpanBytes : 1; }
bool stride_ok(const int64_t stride) { return stride >= 0 && stride < kPngFileMaxStream; }
size_t parts_bytes(const int n_runs, const int64_t stride) { return round16((size_t)n_runs * (size_t)parts_per_run(stride) * sizeof(uint32_t)); }

int launch_crc_parts(const uint8_t *data, const int64_t stride, const long long *sizes, const int n_runs, uint32_t *parts, hipStream_t s)
{
    const int64_t ppr = parts_per_run(stride);
    const unsigned bx = (unsigned)(ppr < kCrcMaxBlocksPerRun ? ppr : kCrcMaxBlocksPerRun);
    hipLaunchKernelGGL(crc_parts_kernel, dim3(bx, (unsigned)n_runs), dim3(kCrcThreads), 0, s, data, stride, sizes, parts, ppr);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int check_crc(const char *fn, const void *data, const int64_t stride, const void *sizes, const int n_runs, const void *crc)
{
    if (!data || !sizes || !crc || n_runs < 0 || !stride_ok(stride)) {
        set_error("%s: bad argument (no NULL pointer, 0 <= stride < 2^31 - 16, n_runs >= 0)", fn);
        return DP_EINVAL;
    }
    return DP_OK;
}

int check_file(const char *fn, const void *streams, const int64_t stream_stride, const void *sizes, const int n_frames, const int n_idat, const void *pre,
               const int64_t pre_stride, const int pre_bytes, const void *post, const int post_bytes, const void *out, const size_t out_bytes,
               const void *offsets)
{
    if (!streams || !sizes || !out || !offsets || n_frames < 0 || !png_file_geometry_ok(stream_stride, pre_bytes, post_bytes) ||
        (pre_bytes && !pre) || (post_bytes && !post) || !(pre_stride == 0 || pre_stride >= pre_bytes) || n_idat < 0 || n_idat > n_frames) {
        set_error("%s: bad argument (no NULL pointer, 0 <= stream_stride < 2^31 - 16, pre_bytes in 0 ... 4096, post_bytes in 0 ... 64, pre_stride 0 or "
                  ">= pre_bytes, n_frames >= 0, n_idat in 0 ... n_frames)", fn);
        return DP_EINVAL;
    }
    const uint64_t bound = png_file_bound(stream_stride, pre_bytes, post_bytes);
    if ((uint64_t)out_bytes / bound < (uint64_t)n_frames) {
        set_error("%s: bad argument (out_bytes of %zu is below %d frames of %llu bytes)", fn, out_bytes, n_frames, (unsigned long long)bound);
        return DP_EINVAL;
    }
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_png_crc32_workspace_bytes(int n_runs, int64_t stride)
{
    if (n_runs < 0 || !stride_ok(stride)) return 0;
    return parts_bytes(n_runs, stride);
}

int dp_png_crc32_u8(const uint8_t *data_dev, int64_t stride, const int64_t *sizes_dev, int n_runs, uint32_t *crc_dev, void *ws_dev,
                    size_t ws_bytes, void *stream)
{
    const char *fn = "dp_png_crc32_u8";
    const int rc = check_crc(fn, data_dev, stride, sizes_dev, n_runs, crc_dev);
    if (rc != DP_OK) return rc;
    if (!ws_dev || ((uintptr_t)ws_dev & 15) || ((uintptr_t)sizes_dev & 7) || ((uintptr_t)crc_dev & 3)) {
        set_error("%s: bad argument (ws_dev 16-byte, sizes_dev 8-byte, crc_dev 4-byte aligned)", fn);
        return DP_EINVAL;
    }
    if (n_runs > 65535) {
        set_error("%s: at most 65535 runs per call, not %d", fn, n_runs);
        return DP_EUNSUPPORTED;
    }
    const size_t need = parts_bytes(n_runs, stride);
    if (ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, need);
        return DP_EWORKSPACE;
    }
    if (n_runs == 0) return DP_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *parts = static_cast<uint32_t *>(ws_dev);
    const long long *sizes = reinterpret_cast<const long long *>(sizes_dev);
    const int lrc = launch_crc_parts(data_dev, stride, sizes, n_runs, parts, s);
    if (lrc != DP_OK) return lrc;
    hipLaunchKernelGGL(crc_join_kernel, dim3((unsigned)n_runs), dim3(64), 0, s, data_dev, stride, sizes, (const uint32_t *)parts, parts_per_run(stride), crc_dev);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int dp_png_crc32_host_u8(const uint8_t *data_host, int64_t stride, const int64_t *sizes_host, int n_runs, uint32_t *crc_host)
{
    const int rc = check_crc("dp_png_crc32_host_u8", data_host, stride, sizes_host, n_runs, crc_host);
    if (rc != DP_OK) return rc;
    for (int r = 0; r < n_runs; ++r)
        crc_host[r] = crc32_bytes(data_host + (size_t)r * (size_t)stride, (size_t)png_file_clamp(sizes_host[r], stride));
    return DP_OK;
}

uint32_t dp_png_crc32_combine_host(uint32_t crc_a, uint32_t crc_b, int64_t len_b)
{
    return crc32_combine(crc_a, crc_b, len_b > 0 ? (uint64_t)len_b : 0u);
}

size_t dp_png_file_bound_bytes(int64_t stream_stride, int pre_bytes, int post_bytes)
{
    if (!png_file_geometry_ok(stream_stride, pre_bytes, post_bytes)) return 0;
    return (size_t)png_file_bound(stream_stride, pre_bytes, post_bytes);
}

size_t dp_png_file_workspace_bytes(int n_frames, int64_t stream_stride)
{
    if (n_frames < 0 || !stride_ok(stream_stride)) return 0;
    return parts_bytes(n_frames, stream_stride);
}

int dp_png_file_assemble_u8(const uint8_t *streams_dev, int64_t stream_stride, const int64_t *sizes_dev, int n_frames, int n_idat,
                            uint32_t seq0, uint32_t seq_step, const uint8_t *pre_dev, int64_t pre_stride, int pre_bytes,
                            const uint8_t *post_dev, int post_bytes, uint8_t *out_dev, size_t out_bytes, int64_t *offsets_dev,
                            void *ws_dev, size_t ws_bytes, void *stream)
{
    const char *fn = "dp_png_file_assemble_u8";
    const int rc = check_file(fn, streams_dev, stream_stride, sizes_dev, n_frames, n_idat, pre_dev, pre_stride, pre_bytes, post_dev, post_bytes, out_dev,
                              out_bytes, offsets_dev);
    if (rc != DP_OK) return rc;
    if (!ws_dev || ((uintptr_t)ws_dev & 15) || ((uintptr_t)sizes_dev & 7) || ((uintptr_t)offsets_dev & 7)) {
        set_error("%s: bad argument (ws_dev 16-byte, sizes_dev and offsets_dev 8-byte aligned)", fn);
        return DP_EINVAL;
    }
    if (n_frames > 65535) {
        set_error("%s: at most 65535 frames per call, not %d", fn, n_frames);
        return DP_EUNSUPPORTED;
    }
    const size_t need = parts_bytes(n_frames, stream_stride);
    if (ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, need);
        return DP_EWORKSPACE;
    }
    if (n_frames == 0) return DP_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *parts = static_cast<uint32_t *>(ws_dev);
    FileArgs a;
    a.streams = streams_dev;
    a.stream_stride = stream_stride;
    a.sizes = reinterpret_cast<const long long *>(sizes_dev);
    a.n_frames = n_frames;
    a.n_idat = n_idat;
    a.seq0 = seq0;
    a.seq_step = seq_step;
    a.pre = pre_dev;
    a.pre_stride = pre_stride;
    a.pre_bytes = pre_bytes;
    a.post = post_dev;
    a.post_bytes = post_bytes;
    a.out = out_dev;
    a.offsets = reinterpret_cast<long long *>(offsets_dev);
    const int lrc = launch_crc_parts(streams_dev, stream_stride, a.sizes, n_frames, parts, s);
    if (lrc != DP_OK) return lrc;
    hipLaunchKernelGGL(file_layout_kernel, dim3(1), dim3(kLayoutThreads), 0, s, a);
    DP_HIP(hipGetLastError());
    const uint64_t words = (png_file_bound(stream_stride, pre_bytes, post_bytes) + 3u) / 4u + 1u;
    const uint64_t bx = (words + kCopyWordsPerBlock - 1) / kCopyWordsPerBlock;
    hipLaunchKernelGGL(file_copy_kernel, dim3((unsigned)(bx < kCopyMaxBlocksPerFrame ? bx : kCopyMaxBlocksPerFrame), (unsigned)n_frames), dim3(kCopyThreads), 0,
                       s, a, (const uint32_t *)parts, parts_per_run(stream_stride));
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int dp_png_file_assemble_host_u8(const uint8_t *streams_host, int64_t stream_stride, const int64_t *sizes_host, int n_frames, int n_idat,
                                 uint32_t seq0, uint32_t seq_step, const uint8_t *pre_host, int64_t pre_stride, int pre_bytes,
                                 const uint8_t *post_host, int post_bytes, uint8_t *out_host, size_t out_bytes, int64_t *offsets_host)
{
    const int rc = check_file("dp_png_file_assemble_host_u8", streams_host, stream_stride, sizes_host, n_frames, n_idat, pre_host, pre_stride, pre_bytes,
                              post_host, post_bytes, out_host, out_bytes, offsets_host);
    if (rc != DP_OK) return rc;
    if (n_frames == 0) return DP_OK;
    png_file_assemble(streams_host, stream_stride, sizes_host, n_frames, n_idat, seq0, seq_step, pre_host, pre_stride, pre_bytes, post_host, post_bytes,
                      out_host, offsets_host);
    return DP_OK;
}

}  // extern "C"
