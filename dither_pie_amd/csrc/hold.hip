// Temporal hold (include/ditherpie_hip_hold.h): cells whose source has not moved keep the indices they show.  The rule is stated by
// host_logic.h: hold_apply; the kernel here writes the same bytes.
//
// hold_kernel<CELL, VEC>   ONE launch per call, grid (ceil(w / 64), ceil(h / 16)), 256 lanes; the loop over the frames is inside.
//   A workgroup owns a tile of 64 x 16 pixels (whole cells for every cell size), each of its four waves a quarter of 32 x 8, and a
//   lane a run of 4 pixels of one row: 12 anchor bytes and 4 held indices in four registers, read once in front of the loop (not at
//   all without state) and written once behind it.
//   Per frame a lane reads the 12 source bytes and 4 fresh indices of its run -- those of frame f + 1 are issued before anything of
//   frame f is looked at, they do not depend on it --, counts its changed pixels, and the cell's count is put together across lanes:
//   cells of 1 need nothing, cells of 2, 4 and 8 lie inside one wave (shuffles), a cell of 16 spans two waves, each of which leaves
//   its half in LDS in front of the frame's barrier.  Refreshed pixels take the frame's bytes (byte masks, no branch); the lane
//   stores its 4 indices of out[f].
//   refreshed[f]: a wave sums its refreshed pixels (shuffles) and leaves the sum in LDS; behind the NEXT frame's barrier lane 0 adds
//   the four sums to refreshed[f] with one 64-bit atomic (none when the sum is 0: the counters are cleared on the stream in front
//   of the launch).  So there is one barrier per frame and one behind the last; both LDS arrays are double-buffered by f & 1, which
//   that one barrier makes safe: a buffer written in frame f is read behind barrier f (or f + 1) and written again in frame f + 2.
//   VEC: every base is 4-byte aligned and w is a multiple of 4, so every run is complete and dword-aligned: dword loads and stores.
//   Otherwise (an odd address, a width that cuts the last run, w < 4) the byte instance: the same registers, filled and stored byte
//   by byte, nothing outside the row touched.
//   A 64 x 114 frame fills 8 workgroups and its call is bound by the latency of one frame after the other, not by bandwidth
//   (DESIGN.md 4.4).
#include "dp_internal.h"

#include "../../include/ditherpie_hip_hold.h"

namespace dp {
namespace {

constexpr int kHoldThreads = 256;
constexpr int kHoldRun = 4;          // pixels of a lane
constexpr int kHoldTileW = 64, kHoldTileH = 16;

struct HoldRun {
    uint32_t s0, s1, s2;   // 12 source (anchor) bytes, little-endian
    uint32_t p;            // 4 indices
};

// byte b (0 .. 11) of a run's colour bytes
__device__ __forceinline__ uint32_t hold_byte(const uint32_t s0, const uint32_t s1, const uint32_t s2, const int b)
{
    const uint32_t wd = b < 4 ? s0 : (b < 8 ? s1 : s2);
    return (wd >> (8 * (b & 3))) & 255u;
}

// nv pixels (0 .. 4; VEC: 0 or 4) of a run: colour bytes at c, indices at p.  Bytes that are not loaded are 0.
template <bool VEC>
__device__ __forceinline__ HoldRun hold_load(const uint8_t *__restrict__ c, const uint8_t *__restrict__ p, const int nv)
{
    HoldRun r{0u, 0u, 0u, 0u};
    if (VEC) {
        // every lane loads (one without pixels from the frame's first run, see `at`) and the bytes are dropped afterwards: a branch
        // around the loads would make the compiler wait for ALL loads in flight where the paths meet, the prefetched ones too
        const uint32_t *__restrict__ c4 = reinterpret_cast<const uint32_t *>(c);
        const uint32_t a = c4[0], b = c4[1], d = c4[2], q = *reinterpret_cast<const uint32_t *>(p);
        r.s0 = nv ? a : 0u, r.s1 = nv ? b : 0u, r.s2 = nv ? d : 0u, r.p = nv ? q : 0u;
    } else {
        uint32_t s[3] = {0u, 0u, 0u};   // (constant indices once unrolled: registers)
#pragma unroll
        for (int b = 0; b < 3 * kHoldRun; ++b)
            if (b < 3 * nv) s[b >> 2] |= (uint32_t)c[b] << (8 * (b & 3));
#pragma unroll
        for (int k = 0; k < kHoldRun; ++k)
            if (k < nv) r.p |= (uint32_t)p[k] << (8 * k);
        r.s0 = s[0], r.s1 = s[1], r.s2 = s[2];
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void hold_store_indices(uint8_t *__restrict__ p, const uint32_t v, const int nv)
{
    if (VEC) {
        if (nv) *reinterpret_cast<uint32_t *>(p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < kHoldRun; ++k)
            if (k < nv) p[k] = (uint8_t)(v >> (8 * k));
    }
}

template <bool VEC>
__device__ __forceinline__ void hold_store_colours(uint8_t *__restrict__ c, const HoldRun &r, const int nv)
{
    if (VEC) {
        if (nv) {
            uint32_t *__restrict__ c4 = reinterpret_cast<uint32_t *>(c);
            c4[0] = r.s0, c4[1] = r.s1, c4[2] = r.s2;
        }
    } else {
#pragma unroll
        for (int b = 0; b < 3 * kHoldRun; ++b)
            if (b < 3 * nv) c[b] = (uint8_t)hold_byte(r.s0, r.s1, r.s2, b);
    }
}

__device__ __forceinline__ uint32_t clip_extent(const int at, const int size, const int limit)   // pixels of [at, at + size) below limit
{
    const int e = limit - at;
    return (uint32_t)(e < 0 ? 0 : (e > size ? size : e));
}

template <int CELL, bool VEC>
__global__ __launch_bounds__(kHoldThreads) void hold_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ planes, const int n_frames,
                                                             const int h, const int w, const uint32_t tol, const uint32_t share256,
                                                             uint8_t *__restrict__ anchor, uint8_t *__restrict__ held, const int has_state,
                                                             uint8_t *__restrict__ out, unsigned long long *__restrict__ refreshed)
{
    __shared__ uint32_t s_half[2][4][2];   // [f & 1][cell of the tile][upper / lower wave]: changed pixels of half a 16-cell
    __shared__ uint32_t s_sum[2][4];       // [f & 1][wave]: refreshed pixels
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wx = wave & 1, wy = wave >> 1, lx = lane & 7, ly = lane >> 3;
    const int x0 = (int)blockIdx.x * kHoldTileW + wx * 32 + lx * kHoldRun;
    const int y = (int)blockIdx.y * kHoldTileH + wy * 8 + ly;
    const int nv = y < h ? (int)clip_extent(x0, kHoldRun, w) : 0;   // the lane's pixels inside the frame
    const size_t hw = (size_t)h * (size_t)w;
    const size_t at = nv ? (size_t)y * (size_t)w + (size_t)x0 : 0;  // the run's first pixel; a lane without pixels points at the
                                                                    // frame's first run (VEC: a complete one), which it may load

    // pixels of the lane's cell(s): CELL 2 has two per run, the others one
    uint32_t cell_px = 0, cell_px_b = 0;
    if (CELL == 2) {
        const uint32_t ch = clip_extent(y & ~1, 2, h);
        cell_px = ch * clip_extent(x0, 2, w);
        cell_px_b = ch * clip_extent(x0 + 2, 2, w);
    } else if (CELL > 2) {
        cell_px = clip_extent(y & ~(CELL - 1), CELL, h) * clip_extent(x0 & ~(CELL - 1), CELL, w);
    }

    HoldRun st{0u, 0u, 0u, 0u};   // anchor bytes and held indices
    if (has_state) st = hold_load<VEC>(anchor + at * 3u, held + at, nv);
    HoldRun even = hold_load<VEC>(src + at * 3u, planes + at, nv), odd{0u, 0u, 0u, 0u};

    // frame f, whose bytes are in `cur`; the loads of frame f + 1 go into `nxt`.  The two register sets swap roles from frame to
    // frame (the loop below is unrolled by two): a copy cur = nxt would wait for the loads it has just issued.
    auto frame = [&](const int f, const HoldRun &cur, HoldRun &nxt) {
        {   // (the last frame loads itself again rather than nothing: no path without loads, for the same reason as in hold_load)
            const size_t o = (size_t)(f + 1 < n_frames ? f + 1 : f) * hw + at;
            nxt = hold_load<VEC>(src + o * 3u, planes + o, nv);
        }
        const bool vote = has_state || f > 0;   // (uniform)
        const int buf = f & 1;
        // changed pixels of the run; bytes outside the frame are 0 on both sides and never differ
        uint32_t ck[kHoldRun];
#pragma unroll
        for (int k = 0; k < kHoldRun; ++k) {
            uint32_t d = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int a = (int)hold_byte(cur.s0, cur.s1, cur.s2, 3 * k + c), b = (int)hold_byte(st.s0, st.s1, st.s2, 3 * k + c);
                const uint32_t e = (uint32_t)(a > b ? a - b : b - a);
                d = e > d ? e : d;
            }
            ck[k] = d > tol ? 1u : 0u;
        }
        uint32_t cnt = ck[0] + ck[1] + ck[2] + ck[3];
        uint32_t cnt_b = 0;
        if (CELL == 2) {
            uint32_t ab = (ck[0] + ck[1]) | ((ck[2] + ck[3]) << 8);
            ab += (uint32_t)__shfl_xor((int)ab, 8);
            cnt = ab & 255u, cnt_b = ab >> 8;
        }
        if (CELL >= 4) {
            cnt += (uint32_t)__shfl_xor((int)cnt, 8);
            cnt += (uint32_t)__shfl_xor((int)cnt, 16);
        }
        if (CELL >= 8) {
            cnt += (uint32_t)__shfl_xor((int)cnt, 1);
            cnt += (uint32_t)__shfl_xor((int)cnt, 32);
        }
        if (CELL == 16) {
            cnt += (uint32_t)__shfl_xor((int)cnt, 2);
            if (vote && (lane & ~4) == 0) s_half[buf][wx * 2 + (lx >> 2)][wy] = cnt;   // lanes 0 and 4: one per half cell
        }
        __syncthreads();
        if (tid == 0 && f > 0) {   // the sums of frame f - 1 are complete behind this barrier
            const uint32_t t = s_sum[buf ^ 1][0] + s_sum[buf ^ 1][1] + s_sum[buf ^ 1][2] + s_sum[buf ^ 1][3];
            if (t) atomicAdd(&refreshed[f - 1], (unsigned long long)t);
        }
        if (CELL == 16) {
            const int cx = wx * 2 + (lx >> 2);
            cnt = vote ? s_half[buf][cx][0] + s_half[buf][cx][1] : 0u;
        }
        bool rk[kHoldRun];
#pragma unroll
        for (int k = 0; k < kHoldRun; ++k) {
            if (!vote)
                rk[k] = true;
            else if (CELL == 1)
                rk[k] = ck[k] != 0u;   // (a cell of one pixel: 256 >= share256 always)
            else if (CELL == 2)
                rk[k] = k < 2 ? hold_refreshes(cnt, cell_px, share256) : hold_refreshes(cnt_b, cell_px_b, share256);
            else
                rk[k] = hold_refreshes(cnt, cell_px, share256);
        }
        const uint32_t e0 = rk[0] ? ~0u : 0u, e1 = rk[1] ? ~0u : 0u, e2 = rk[2] ? ~0u : 0u, e3 = rk[3] ? ~0u : 0u;
        const uint32_t m0 = (e0 & 0x00FFFFFFu) | (e1 & 0xFF000000u), m1 = (e1 & 0x0000FFFFu) | (e2 & 0xFFFF0000u),
                       m2 = (e2 & 0x000000FFu) | (e3 & 0xFFFFFF00u);
        const uint32_t mp = (e0 & 0x000000FFu) | (e1 & 0x0000FF00u) | (e2 & 0x00FF0000u) | (e3 & 0xFF000000u);
        st.s0 = (st.s0 & ~m0) | (cur.s0 & m0);
        st.s1 = (st.s1 & ~m1) | (cur.s1 & m1);
        st.s2 = (st.s2 & ~m2) | (cur.s2 & m2);
        st.p = (st.p & ~mp) | (cur.p & mp);
        if (nv) hold_store_indices<VEC>(out + (size_t)f * hw + at, st.p, nv);
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < kHoldRun; ++k) r += (rk[k] && k < nv) ? 1u : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) r += (uint32_t)__shfl_xor((int)r, off);
        if (lane == 0) s_sum[buf][wave] = r;
    };
    for (int f = 0; f < n_frames; f += 2) {
        frame(f, even, odd);
        if (f + 1 < n_frames) frame(f + 1, odd, even);   // (uniform: the barrier inside is reached by all lanes or none)
    }
    if (nv) {
        hold_store_colours<VEC>(anchor + at * 3u, st, nv);
        hold_store_indices<VEC>(held + at, st.p, nv);
    }
    __syncthreads();
    if (tid == 0) {
        const int buf = (n_frames - 1) & 1;
        const uint32_t t = s_sum[buf][0] + s_sum[buf][1] + s_sum[buf][2] + s_sum[buf][3];
        if (t) atomicAdd(&refreshed[n_frames - 1], (unsigned long long)t);
    }
}

template <int CELL>
void launch_hold_cell(const bool vec, const dim3 grid, hipStream_t s, const dp_hold_args &a)
{
    unsigned long long *refreshed = reinterpret_cast<unsigned long long *>(a.refreshed_dev);
    if (vec)
        hipLaunchKernelGGL((hold_kernel<CELL, true>), grid, dim3(kHoldThreads), 0, s, a.src_dev, a.planes_dev, (int)a.n_frames, a.h, a.w, (uint32_t)a.tol,
                           (uint32_t)a.share256, a.anchor_dev, a.held_dev, a.has_state ? 1 : 0, a.out_dev, refreshed);
    else
        hipLaunchKernelGGL((hold_kernel<CELL, false>), grid, dim3(kHoldThreads), 0, s, a.src_dev, a.planes_dev, (int)a.n_frames, a.h, a.w, (uint32_t)a.tol,
                           (uint32_t)a.share256, a.anchor_dev, a.held_dev, a.has_state ? 1 : 0, a.out_dev, refreshed);
}

int launch_hold(const dp_hold_args &a)
{
    hipStream_t s = (hipStream_t)a.stream;
    ProfMark *pm = prof_begin(s);   // (nullptr unless dp_profile_enable is on: nothing is recorded then)
    DP_HIP(hipMemsetAsync(a.refreshed_dev, 0, (size_t)a.n_frames * sizeof(int64_t), s));
    const bool vec = (((uintptr_t)a.src_dev | (uintptr_t)a.planes_dev | (uintptr_t)a.anchor_dev | (uintptr_t)a.held_dev | (uintptr_t)a.out_dev |
                       (uintptr_t)a.w) & 3u) == 0;
    const dim3 grid((unsigned)((a.w + kHoldTileW - 1) / kHoldTileW), (unsigned)((a.h + kHoldTileH - 1) / kHoldTileH));
    switch (a.cell) {
    case 1: launch_hold_cell<1>(vec, grid, s, a); break;
    case 2: launch_hold_cell<2>(vec, grid, s, a); break;
    case 4: launch_hold_cell<4>(vec, grid, s, a); break;
    case 8: launch_hold_cell<8>(vec, grid, s, a); break;
    default: launch_hold_cell<16>(vec, grid, s, a); break;
    }
    DP_HIP(hipGetLastError());
    prof_end(pm, s);
    return DP_OK;
}

bool overlap(const void *a, const size_t na, const void *b, const size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

const char *const kHoldRule[] = {"", "n_frames must not be negative", "h and w must be >= 1 and h * w below 2^31", "cell must be one of 1, 2, 4, 8, 16",
                                 "tol must lie in 0 .. 255", "share256 must lie in 0 .. 256", "at most 65535 frames per call"};

// the checks both entry points share -> DP_OK, or the refusal (its message names fn)
int check_hold(const char *fn, const dp_hold_args *a)
{
    if (!a || a->struct_size != sizeof(dp_hold_args)) {
        set_error("%s: bad argument (a NULL descriptor or a struct_size that is not %zu)", fn, sizeof(dp_hold_args));
        return DP_EINVAL;
    }
    if (const int bad = hold_rule(a->n_frames, a->h, a->w, a->cell, a->tol, a->share256)) {
        set_error("%s: %s (n_frames %lld, %d x %d, cell %d, tol %d, share256 %d)", fn, kHoldRule[bad], (long long)a->n_frames, a->h, a->w, a->cell,
                  a->tol, a->share256);
        return bad == 6 ? DP_EUNSUPPORTED : DP_EINVAL;
    }
    if (a->n_frames == 0) return DP_OK;
    if (!a->src_dev || !a->planes_dev || !a->anchor_dev || !a->held_dev || !a->out_dev || !a->refreshed_dev) {
        set_error("%s: bad argument (a NULL buffer)", fn);
        return DP_EINVAL;
    }
    if ((uintptr_t)a->refreshed_dev & 7u) {
        set_error("%s: refreshed_dev must be 8-byte aligned", fn);
        return DP_EINVAL;
    }
    const size_t px = (size_t)a->h * (size_t)a->w, n = (size_t)a->n_frames;
    const struct { const void *p; size_t bytes; } in[2] = {{a->src_dev, n * px * 3u}, {a->planes_dev, n * px}},
                                                  rw[4] = {{a->out_dev, n * px}, {a->anchor_dev, px * 3u}, {a->held_dev, px}, {a->refreshed_dev, n * 8u}};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j)
            if (overlap(rw[i].p, rw[i].bytes, in[j].p, in[j].bytes)) {
                set_error("%s: bad argument (out_dev, the state and refreshed_dev must not overlap src_dev or planes_dev)", fn);
                return DP_EINVAL;
            }
        for (int j = i + 1; j < 4; ++j)
            if (overlap(rw[i].p, rw[i].bytes, rw[j].p, rw[j].bytes)) {
                set_error("%s: bad argument (out_dev, anchor_dev, held_dev and refreshed_dev must not overlap each other)", fn);
                return DP_EINVAL;
            }
    }
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

int dp_hold_u8(const dp_hold_args *a)
{
    if (const int rc = check_hold("dp_hold_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    return launch_hold(*a);
}

int dp_hold_host_u8(const dp_hold_args *a)
{
    if (const int rc = check_hold("dp_hold_host_u8", a)) return rc;
    if (a->n_frames == 0) return DP_OK;
    hold_apply(a->src_dev, a->planes_dev, a->n_frames, a->h, a->w, a->cell, a->tol, a->share256, a->anchor_dev, a->held_dev, a->has_state != 0,
               a->out_dev, a->refreshed_dev);
    return DP_OK;
}

int dp_hold_state_bytes(int h, int w, size_t *anchor_bytes, size_t *held_bytes)
{
    if (!anchor_bytes || !held_bytes || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) {
        set_error("dp_hold_state_bytes: bad argument (pointers, h and w >= 1, h * w below 2^31)");
        return DP_EINVAL;
    }
    *held_bytes = (size_t)h * (size_t)w;
    *anchor_bytes = 3u * *held_bytes;
    return DP_OK;
}

}  // extern "C"
