// PNG-8 output (include/ditherpie_hip_png.h): the zlib stream of planes of palette indices.  The stream is stated by
// host_logic.h: png_deflate_encode; the kernels here write the same bytes, and the pieces that could drift (the filtered
// byte at an offset, the trigram hash, the fixed-Huffman bits of a token, the size of a segment per block type) are the
// host's own functions compiled for the device.
//
// png_segment_kernel   one wave (a workgroup of 64) owns one segment at a time, grid stride over the segments of the batch.
//                      1. The segment's filtered bytes are packed from the plane into LDS (one division by the row length
//                         per byte, the loads of a lane independent of each other); the Adler sums of the segment are taken
//                         on the way.
//                      2. 64 positions a step.  Candidates: the hash heads (4096 x 16 bit in LDS) give the last position
//                         before the step, the 64 hashes of the step are compared lane against lane (64 readlanes) for the
//                         last position inside it; the highest lane of a bucket then inserts.  A step the match before
//                         covers entirely still inserts (candidates are a function of the bytes alone) but compares nothing.
//                      3. Match lengths per lane from LDS, four bytes a read pair.
//                      4. Greedy selection on the ballot of 'length >= 3': from the current position the next set bit is the
//                         next match, everything before it is literals; one shuffle per match taken, nothing per literal.
//                      5. Bits per token (fixed Huffman) -> wave prefix sum -> OR into a small LDS stage -> whole words to the
//                         segment's workspace slot, up to the slot's size (beyond it the stored block has won already).
//                      6. The segment's size as stored and as fixed Huffman decide (png_segment_choice); a stored segment
//                         overwrites its slot from LDS.  The slot then holds the segment's final bytes, realigning block
//                         included, and rec[] its length and Adler sums.
//                      This kernel writes stored and fixed blocks only; png_segment_dyn_kernel below adds dynamic ones.
//                      LDS: 32784 (segment) + 8192 (heads) + 288 (stage) = 41264 bytes, so 3 workgroups per CU of the 160
//                      KiB, 768 segments in flight on 256 CUs.  One 1080p frame at depth 8 is 64 segments of 32 KiB: a
//                      quarter of the CUs, one wave each, and the serial part of a segment (steps 2 ... 5, <= 512 steps) is
//                      the frame's latency.  At 8 KiB it is 254 segments with a quarter of the steps each: a single frame
//                      fills the CUs once, a batch of a few frames fills the residency.  The default is 8 KiB
//                      (DESIGN.md 4.4 has the sizes measured with the host statement that go with it).
//                      Loops: bytes of a segment / 64 <= 512 per lane; steps <= 512; lane compare 64; a match length <= 65
//                      read pairs; selection <= 22 matches a step (each advances >= 3 positions); scans 6 levels.
// png_layout_kernel    one wave per frame: exclusive prefix over the segments' byte lengths (wave scan, 64 a step), the
//                      Adler-32 of the frame from the segments' (sum, weighted sum) pairs -- every term is reduced mod
//                      65521 before it is multiplied or added, so nothing exceeds 2^32 * 2^16 in 64 bits --, the 2-byte
//                      header, the 4-byte trailer, sizes[f].  Loop: ceil(n_seg / 64).
// png_pack_kernel      grid (blocks per frame, frames): a workgroup copies one segment's slot to its place in `out`, byte by
//                      byte (segments are byte-aligned: no shifting), grid stride over the frame's segments.  Plain
//                      stores, no atomics, nothing read from `out`.  Loops: n_seg / gridDim.x, slot bytes / 256.
//
// Dynamic-Huffman blocks (include/ditherpie_hip_png_dyn.h, host_logic.h: png_deflate_encode_dyn).  png_layout_kernel and
// png_pack_kernel are reused as they are; png_segment_kernel is untouched (a second kernel, not a branch in its step loop).
// png_segment_dyn_kernel   one wave per segment, as above.
//                      Pass 1: steps 1 ... 4 as above; instead of emitting, a step counts its tokens into LDS histograms
//                         (286 + 30 counters, integer LDS atomics: 64 lanes meet on one counter only where 64 equal literals
//                         follow each other without a match, which the matcher turns into one token after three bytes), adds
//                         up the fixed-Huffman bits and the extra bits per lane, and writes one 32-bit word per token,
//                         compacted by the step's prefix count, to the segment's token area (4 * seg bytes of workspace).
//                      Build: per alphabet (literal/length, distance, then the code-length alphabet over the run-length
//                         coded lengths) the keys count << 9 | symbol are rank-sorted by the wave (each lane counts the
//                         keys below its own: <= 5 keys a lane x 286 broadcast reads), lane 0 runs the host's merge, limit
//                         and assignment (png_code_lengths_sorted: <= 285 merges, <= 286 depths, <= 286 fix-up rounds of
//                         <= 15) and the run-length coding (png_cl_sequence: <= 316 lengths).
//                      Choose: the dynamic block's bits are summed by the wave from the histograms, the extra bits and the
//                         lengths (316 symbols and <= 316 sequence entries, 5 a lane); png_segment_choice with three sizes.
//                      Pass 2: only the chosen type is written.  Stored: the bytes from LDS.  Fixed or dynamic: the block
//                         header (one step: 14 bits and HCLEN x 3), the code-length sequence (<= 5 steps), the token words
//                         64 a step (<= seg / 64 steps ... <= 512), end-of-block, the realigning block.  A dynamic token is
//                         up to 15 + 5 + 15 + 13 = 48 bits, so the stage is 128 words (31 carried bits + 64 x 48 = 97 words,
//                         and a token's three-word span ends at word 97) and a step moves up to 97 words, two a lane.
//                         Slot writes stay clipped at slot_words; token writes at the token area's seg words.
//                      LDS: 32784 (segment) + 8192 (heads) + 512 (stage) + 1264 (histograms) + 1340 (codes) + 336
//                      (lengths) + 632 (sequence) + 80 (code-length counts) + 4576 (builder) = 49716 bytes <= 54613: three
//                      workgroups per CU as before.
// png_code_lengths_kernel  dp_png_code_lengths_u8: one wave per histogram, grid stride; the same wave_code_lengths.
#include "dp_internal.h"

#include "../../include/ditherpie_hip_png.h"
#include "../../include/ditherpie_hip_png_dyn.h"

namespace dp {
namespace {

constexpr int kSegWords = kPngSegMax / 4 + 4;     // the segment and 16 bytes a match comparison may read past its end
constexpr int kHeads = 1 << kPngHashBits;
constexpr int kStageWords = 72;                   // 31 carried bits + 64 tokens of <= 31 bits: 63 words, and one to spill
constexpr int kSegMaxBlocks = 256 * 3 * 4;        // 3 resident workgroups per CU, four rounds; the rest by grid stride
constexpr int kPackThreads = 256;
constexpr int kPackMaxBlocksPerFrame = 1024;

struct SegRec {
    uint32_t len;   // bytes of the segment in its slot
    uint32_t s1;    // sum of its filtered bytes mod 65521
    uint32_t s2;    // sum of (n - i) * byte[i] mod 65521
    uint32_t off;   // byte offset of the segment behind the frame's 2-byte header (the layout kernel's)
};

__device__ __forceinline__ unsigned long long low_mask(const uint32_t k) { return k >= 64u ? ~0ull : (1ull << k) - 1ull; }

__device__ __forceinline__ uint32_t lds_read_u32_at(const uint32_t *s_w, const uint32_t byte_addr)   // unaligned, from two words
{
    const uint32_t i = byte_addr >> 2, sh = (byte_addr & 3u) * 8u;
    const unsigned long long two = ((unsigned long long)s_w[i + 1] << 32) | s_w[i];
    return (uint32_t)(two >> sh);
}

__global__ __launch_bounds__(64) void png_segment_kernel(const uint8_t *__restrict__ planes, const int h, const int w, const int depth,
                                                         const uint32_t rb, const uint32_t F, const uint32_t seg, const int n_seg,
                                                         const int total_segs, uint8_t *__restrict__ slots, const long long slot_bytes,
                                                         SegRec *__restrict__ rec)
{
    __shared__ uint32_t s_w[kSegWords];
    __shared__ uint16_t heads[kHeads];
    __shared__ uint32_t stage[kStageWords];
    uint8_t *s_b = reinterpret_cast<uint8_t *>(s_w);
    const uint32_t lane = threadIdx.x;
    const uint32_t slot_words = (uint32_t)(slot_bytes >> 2);
    const size_t plane_bytes = (size_t)h * (size_t)w;

    for (int id = (int)blockIdx.x; id < total_segs; id += (int)gridDim.x) {
        const int f = id / n_seg, j = id - f * n_seg;
        const uint32_t at = (uint32_t)j * seg;
        const uint32_t n = seg < F - at ? seg : F - at;
        const bool last = j == n_seg - 1;
        const uint8_t *__restrict__ plane = planes + (size_t)f * plane_bytes;
        uint8_t *__restrict__ slot_b = slots + (size_t)id * (size_t)slot_bytes;
        uint32_t *__restrict__ slot = reinterpret_cast<uint32_t *>(slot_b);

        __syncthreads();   // (the segment before is done with the arrays)
        unsigned long long s1 = 0, s2 = 0;
#pragma unroll 4
        for (uint32_t i = lane; i < n; i += 64u) {   // <= 512
            const uint32_t o = at + i, r = o / rb;
            const uint32_t b = png_filtered_byte(plane, w, depth, r, o - r * rb);
            s_b[i] = (uint8_t)b;
            s1 += b;
            s2 += (unsigned long long)(n - i) * b;
        }
        for (uint32_t i = lane; i < (uint32_t)kHeads; i += 64u) heads[i] = (uint16_t)kPngNoCand;
        for (uint32_t i = lane; i < (uint32_t)kStageWords; i += 64u) stage[i] = 0u;
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_down(s1, off);
            s2 += __shfl_down(s2, off);
        }
        __syncthreads();
        if (lane == 0) stage[0] = (last ? 1u : 0u) | (1u << 1);   // BFINAL, BTYPE 01
        __syncthreads();

        unsigned long long bitpos = 3;   // of the block, from the slot's first bit (uniform)
        uint32_t stage_word = 0;         // the slot word stage[0] stands for (uniform)
        uint32_t skip = 0;               // the first position the matches taken so far do not cover (uniform)

        // ORs a token in at bit `where`, then moves the stage's whole words to the slot; `more` = the new bit position
        auto emit = [&](const uint32_t bits, const int nb, const unsigned long long where, const unsigned long long more, const bool all) {
            if (nb > 0) {
                const uint32_t rel = (uint32_t)(where - 32ull * stage_word), wi = rel >> 5;
                const unsigned long long v = (unsigned long long)bits << (rel & 31u);
                atomicOr(&stage[wi], (uint32_t)v);
                if (v >> 32) atomicOr(&stage[wi + 1u], (uint32_t)(v >> 32));
            }
            __syncthreads();
            uint32_t full = (uint32_t)(more >> 5) - stage_word;           // <= 63
            const uint32_t keep = all ? 0u : stage[full];                  // the word still being filled
            if (all && (more & 31ull)) ++full;
            const uint32_t mine = lane < full ? stage[lane] : 0u;
            __syncthreads();
            if (lane < full && stage_word + lane < slot_words) slot[stage_word + lane] = mine;
            stage[lane] = lane == 0 ? keep : 0u;
            if (lane < (uint32_t)kStageWords - 64u) stage[64u + lane] = 0u;
            __syncthreads();
            stage_word += full;
        };

        for (uint32_t base = 0; base < n; base += 64u) {   // <= 512
            const uint32_t p = base + lane;
            const uint32_t cnt = n - base < 64u ? n - base : 64u;
            const bool valid = p + 2u < n;
            const uint32_t b0 = p < n ? s_b[p] : 0u;
            const uint32_t hv = valid ? png_hash3(b0, s_b[p + 1u], s_b[p + 2u]) : 0x10000u + lane;   // (no other lane's value)
            uint32_t q = valid ? (uint32_t)heads[hv & (uint32_t)(kHeads - 1)] : kPngNoCand;
            bool later = false;
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)hv, k);
                if (hk == hv) {
                    if ((uint32_t)k < lane) q = base + (uint32_t)k;
                    else if ((uint32_t)k > lane) later = true;
                }
            }
            __syncthreads();   // (every lane has read the heads)
            if (valid && !later) heads[hv] = (uint16_t)p;

            uint32_t len = 0;
            if (skip < base + cnt && valid && q != kPngNoCand && p >= skip) {
                const uint32_t maxlen = n - p < 258u ? n - p : 258u;
                for (uint32_t k = 0; k < maxlen; k += 4u) {   // <= 65
                    const uint32_t x = lds_read_u32_at(s_w, q + k) ^ lds_read_u32_at(s_w, p + k);
                    if (x) {
                        len = k + ((uint32_t)__builtin_ctz(x) >> 3);
                        break;
                    }
                    len = k + 4u;
                }
                len = len < maxlen ? len : maxlen;
            }
            const unsigned long long M = __ballot(len >= 3u);

            const uint32_t start = skip > base ? (skip - base < 64u ? skip - base : 64u) : 0u;
            uint32_t pos = start;
            unsigned long long sel = 0, cov = 0;
            for (int it = 0; it < 22 && pos < cnt; ++it) {
                const unsigned long long rest = M >> pos;
                if (!rest) break;
                pos += (uint32_t)__builtin_ctzll(rest);
                const uint32_t L = (uint32_t)__shfl((int)len, (int)pos);
                sel |= 1ull << pos;
                cov |= low_mask(pos + L) & ~low_mask(pos + 1u);
                pos += L;
                skip = base + pos;
            }
            const unsigned long long T = low_mask(cnt) & ~low_mask(start) & ~cov;
            const bool is_tok = (T >> lane) & 1ull, is_match = (sel >> lane) & 1ull;

            PngBits t;
            t.bits = 0u;
            t.nb = 0;
            if (is_tok) t = is_match ? png_fixed_match((int)len, (int)(p - q)) : png_fixed_literal(b0);
            uint32_t incl = (uint32_t)t.nb;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(incl, off);
                if (lane >= (uint32_t)off) incl += up;
            }
            const uint32_t step_bits = __shfl(incl, 63);
            emit(t.bits, t.nb, bitpos + incl - (uint32_t)t.nb, bitpos + step_bits, false);
            bitpos += step_bits;
        }
        bitpos += 7;   // end of block: seven zero bits, which the stage holds already

        const uint32_t stored_bytes = png_stored_segment_bytes(n, last), fixed_bytes = png_huffman_segment_bytes(bitpos, last);
        const int type = png_segment_choice(stored_bytes, fixed_bytes);
        if (type == kPngFixed) {   // (fixed_bytes < stored_bytes <= slot_bytes)
            if (!last) {
                const unsigned long long aligned = (bitpos + 3ull + 7ull) & ~7ull;
                emit(0xFFFF0000u, lane == 0 ? 32 : 0, aligned, aligned + 32ull, true);   // 00 00 FF FF
            } else {
                emit(0u, 0, bitpos, bitpos, true);
            }
        } else {
            // The fixed bits written above went to this slot as dwords from other lanes of this wave; the bytes below replace
            // them.  A wave's stores to one address complete in issue order; the fence makes that a stated wait (vmcnt) rather
            // than a property relied on.
            __threadfence_block();
            __syncthreads();
            if (lane == 0) {
                slot_b[0] = last ? 1 : 0;
                slot_b[1] = (uint8_t)(n & 0xFFu);
                slot_b[2] = (uint8_t)(n >> 8);
                slot_b[3] = (uint8_t)(~n & 0xFFu);
                slot_b[4] = (uint8_t)((~n >> 8) & 0xFFu);
                if (!last) {
                    slot_b[5u + n] = 0x00;
                    slot_b[6u + n] = 0x00;
                    slot_b[7u + n] = 0x00;
                    slot_b[8u + n] = 0xFF;
                    slot_b[9u + n] = 0xFF;
                }
            }
            for (uint32_t i = lane; i < n; i += 64u) slot_b[5u + i] = s_b[i];   // <= 512
        }
        if (lane == 0) {
            SegRec r;
            r.len = type == kPngFixed ? fixed_bytes : stored_bytes;
            r.s1 = (uint32_t)(s1 % kAdlerMod);
            r.s2 = (uint32_t)(s2 % kAdlerMod);
            r.off = 0u;
            rec[id] = r;
        }
    }
}

__global__ __launch_bounds__(64) void png_layout_kernel(SegRec *__restrict__ rec, const int n_seg, const uint32_t F, const uint32_t seg,
                                                        uint8_t *__restrict__ out, const long long out_stride, long long *__restrict__ sizes)
{
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    SegRec *__restrict__ R = rec + (size_t)f * (size_t)n_seg;
    unsigned long long carry = 0;
    uint32_t A = 1u, B = 0u;
    for (int base = 0; base < n_seg; base += 64) {
        const int j = base + lane;
        const bool valid = j < n_seg;
        uint32_t len = 0, s1 = 0, s2 = 0, nj = 0;
        if (valid) {
            const SegRec r = R[j];
            len = r.len;
            s1 = r.s1;
            s2 = r.s2;
            const uint32_t at = (uint32_t)j * seg;
            nj = seg < F - at ? seg : F - at;
        }
        unsigned long long incl = len;
        uint32_t incl1 = s1;   // (64 * 65520 fits)
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(incl, off);
            const uint32_t up1 = __shfl_up(incl1, off);
            if (lane >= off) {
                incl += up;
                incl1 += up1;
            }
        }
        const uint32_t a_before = (A + (incl1 - s1)) % kAdlerMod;
        unsigned long long term = ((unsigned long long)nj * a_before + s2) % kAdlerMod;
        for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off);
        term = __shfl(term, 0);
        B = (uint32_t)((B + term) % kAdlerMod);
        A = (A + __shfl(incl1, 63)) % kAdlerMod;
        if (valid) R[j].off = (uint32_t)(carry + incl - len);
        carry += __shfl(incl, 63);
    }
    if (lane == 0) {
        uint8_t *__restrict__ dst = out + (size_t)f * (size_t)out_stride;
        const unsigned long long limit = (unsigned long long)out_stride, t = 2ull + carry;   // (the bound keeps t + 4 <= limit; checked all the same)
        if (t + 4ull <= limit) {
            dst[0] = 0x78;
            dst[1] = 0x01;
            dst[t] = (uint8_t)(B >> 8);
            dst[t + 1] = (uint8_t)B;
            dst[t + 2] = (uint8_t)(A >> 8);
            dst[t + 3] = (uint8_t)A;
        }
        sizes[f] = (long long)(t + 4ull);
    }
}

__global__ __launch_bounds__(kPackThreads) void png_pack_kernel(const SegRec *__restrict__ rec, const int n_seg, const uint8_t *__restrict__ slots,
                                                                 const long long slot_bytes, uint8_t *__restrict__ out, const long long out_stride)
{
    const int f = (int)blockIdx.y;
    const size_t row = (size_t)f * (size_t)n_seg;
    uint8_t *__restrict__ dst = out + (size_t)f * (size_t)out_stride;
    const unsigned long long limit = (unsigned long long)out_stride;
    for (int j = (int)blockIdx.x; j < n_seg; j += (int)gridDim.x) {
        const SegRec r = rec[row + (size_t)j];
        const uint8_t *__restrict__ src = slots + (row + (size_t)j) * (size_t)slot_bytes;
        const uint32_t len = r.len < (uint32_t)slot_bytes ? r.len : (uint32_t)slot_bytes;
        const unsigned long long to = 2ull + r.off;
        for (uint32_t i = threadIdx.x; i < len; i += kPackThreads)
            if (to + i < limit) dst[to + i] = src[i];
    }
}

// ---- dynamic-Huffman blocks ---------------------------------------------------------------------------------------------
constexpr int kDynStageWords = 128;

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, const uint32_t lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(v, off);
        if (lane >= (uint32_t)off) v += up;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return __shfl(v, 0);
}

// Rules (a) ... (e) by one wave (a workgroup of 64): sc.keys[0 .. m) hold png_code_key(count, symbol) and are visible to the
// wave; lengths[0 .. m) (LDS) receive the result, visible on return.
__device__ void wave_code_lengths(PngCodeScratch &sc, const int m, const int L, uint8_t *lengths, const uint32_t lane)
{
    int used = 0;
    for (int s0 = 0; s0 < m; s0 += 64) {   // <= 5
        const int s = s0 + (int)lane;
        used += __popcll(__ballot(s < m && sc.keys[s] < kPngUnusedKey));
    }
    if (used < 2) {
        __syncthreads();
        if (lane == 0) png_pad_keys(sc.keys, m);
        used = 2;
        __syncthreads();
    }
    for (int s = (int)lane; s < m; s += 64) {   // <= 5 keys a lane, every key read by all lanes at once (a broadcast)
        const uint32_t key = sc.keys[s];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += sc.keys[j] < key;   // <= 286 (keys are distinct: the symbol is in them)
        sc.sorted[rank] = key;
    }
    __syncthreads();
    if (lane == 0) png_code_lengths_sorted(sc.sorted, used, m, L, lengths, sc.w, sc.lp, sc.ip);
    __syncthreads();
}

__global__ __launch_bounds__(64) void png_code_lengths_kernel(const uint32_t *__restrict__ counts, const int n_alphabets, const int m, const int L,
                                                              uint8_t *__restrict__ lengths)
{
    __shared__ PngCodeScratch sc;
    __shared__ uint8_t lens[kPngLit + 2];
    const uint32_t lane = threadIdx.x;
    for (int a = (int)blockIdx.x; a < n_alphabets; a += (int)gridDim.x) {
        __syncthreads();
        for (int s = (int)lane; s < m; s += 64) sc.keys[s] = png_code_key(counts[(size_t)a * (size_t)m + (size_t)s], (uint32_t)s);
        __syncthreads();
        wave_code_lengths(sc, m, L, lens, lane);
        for (int s = (int)lane; s < m; s += 64) lengths[(size_t)a * (size_t)m + (size_t)s] = lens[s];
    }
}

__global__ __launch_bounds__(64) void png_segment_dyn_kernel(const uint8_t *__restrict__ planes, const int h, const int w, const int depth,
                                                             const uint32_t rb, const uint32_t F, const uint32_t seg, const int n_seg,
                                                             const int total_segs, uint8_t *__restrict__ slots, const long long slot_bytes,
                                                             uint32_t *__restrict__ token_area, SegRec *__restrict__ rec)
{
    __shared__ uint32_t s_w[kSegWords];
    __shared__ uint16_t heads[kHeads];
    __shared__ uint32_t stage[kDynStageWords];
    __shared__ uint32_t hist[kPngLens];
    __shared__ uint32_t codes[kPngLens + kPngCl];
    __shared__ uint8_t lens[kPngLens + kPngCl + 1];
    __shared__ uint16_t seq[kPngLens];
    __shared__ uint32_t cl_counts[kPngCl + 1];
    __shared__ PngCodeScratch sc;
    __shared__ int s_head[4];   // hlit, hdist, hclen, nseq
    static_assert(sizeof(uint32_t) * (kSegWords + kDynStageWords + 2 * kPngLens + 2 * kPngCl + 1) + sizeof(uint16_t) * (kHeads + kPngLens) +
                          (kPngLens + kPngCl + 1) + sizeof(PngCodeScratch) + 16 <= 54613,
                  "three workgroups per CU");
    uint8_t *s_b = reinterpret_cast<uint8_t *>(s_w);
    const uint32_t lane = threadIdx.x;
    const uint32_t slot_words = (uint32_t)(slot_bytes >> 2);
    const size_t plane_bytes = (size_t)h * (size_t)w;

    for (int id = (int)blockIdx.x; id < total_segs; id += (int)gridDim.x) {
        const int f = id / n_seg, j = id - f * n_seg;
        const uint32_t at = (uint32_t)j * seg;
        const uint32_t n = seg < F - at ? seg : F - at;
        const bool last = j == n_seg - 1;
        const uint8_t *__restrict__ plane = planes + (size_t)f * plane_bytes;
        uint8_t *__restrict__ slot_b = slots + (size_t)id * (size_t)slot_bytes;
        uint32_t *__restrict__ slot = reinterpret_cast<uint32_t *>(slot_b);
        uint32_t *tokens = token_area + (size_t)id * (size_t)seg;   // seg words (read back in pass 2: not __restrict__)

        __syncthreads();   // (the segment before is done with the arrays)
        unsigned long long s1 = 0, s2 = 0;
#pragma unroll 4
        for (uint32_t i = lane; i < n; i += 64u) {   // <= 512
            const uint32_t o = at + i, r = o / rb;
            const uint32_t b = png_filtered_byte(plane, w, depth, r, o - r * rb);
            s_b[i] = (uint8_t)b;
            s1 += b;
            s2 += (unsigned long long)(n - i) * b;
        }
        for (uint32_t i = lane; i < (uint32_t)kHeads; i += 64u) heads[i] = (uint16_t)kPngNoCand;
        for (uint32_t i = lane; i < (uint32_t)kPngLens; i += 64u) hist[i] = 0u;   // <= 5
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_down(s1, off);
            s2 += __shfl_down(s2, off);
        }
        __syncthreads();

        // ---- pass 1: tokens, histograms, bit totals
        uint32_t skip = 0;    // the first position the matches taken so far do not cover (uniform)
        uint32_t ntok = 0;    // tokens written so far (uniform)
        unsigned long long my_fixed = 0, my_extra = 0;
        for (uint32_t base = 0; base < n; base += 64u) {   // <= 512
            const uint32_t p = base + lane;
            const uint32_t cnt = n - base < 64u ? n - base : 64u;
            const bool valid = p + 2u < n;
            const uint32_t b0 = p < n ? s_b[p] : 0u;
            const uint32_t hv = valid ? png_hash3(b0, s_b[p + 1u], s_b[p + 2u]) : 0x10000u + lane;   // (no other lane's value)
            uint32_t q = valid ? (uint32_t)heads[hv & (uint32_t)(kHeads - 1)] : kPngNoCand;
            bool later = false;
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)hv, k);
                if (hk == hv) {
                    if ((uint32_t)k < lane) q = base + (uint32_t)k;
                    else if ((uint32_t)k > lane) later = true;
                }
            }
            __syncthreads();   // (every lane has read the heads)
            if (valid && !later) heads[hv] = (uint16_t)p;

            uint32_t len = 0;
            if (skip < base + cnt && valid && q != kPngNoCand && p >= skip) {
                const uint32_t maxlen = n - p < 258u ? n - p : 258u;
                for (uint32_t k = 0; k < maxlen; k += 4u) {   // <= 65
                    const uint32_t x = lds_read_u32_at(s_w, q + k) ^ lds_read_u32_at(s_w, p + k);
                    if (x) {
                        len = k + ((uint32_t)__builtin_ctz(x) >> 3);
                        break;
                    }
                    len = k + 4u;
                }
                len = len < maxlen ? len : maxlen;
            }
            const unsigned long long M = __ballot(len >= 3u);

            const uint32_t start = skip > base ? (skip - base < 64u ? skip - base : 64u) : 0u;
            uint32_t pos = start;
            unsigned long long sel = 0, cov = 0;
            for (int it = 0; it < 22 && pos < cnt; ++it) {
                const unsigned long long rest = M >> pos;
                if (!rest) break;
                pos += (uint32_t)__builtin_ctzll(rest);
                const uint32_t L = (uint32_t)__shfl((int)len, (int)pos);
                sel |= 1ull << pos;
                cov |= low_mask(pos + L) & ~low_mask(pos + 1u);
                pos += L;
                skip = base + pos;
            }
            const unsigned long long T = low_mask(cnt) & ~low_mask(start) & ~cov;
            const bool is_tok = (T >> lane) & 1ull, is_match = (sel >> lane) & 1ull;

            if (is_tok) {
                const uint32_t word = is_match ? png_token_match((int)len, (int)(p - q)) : png_token_literal(b0);
                uint32_t lit_sym;
                int dist_sym, eb, fb;
                png_token_symbols(word, lit_sym, dist_sym, eb, fb);
                atomicAdd(&hist[lit_sym], 1u);
                if (dist_sym >= 0) atomicAdd(&hist[kPngLit + dist_sym], 1u);
                my_extra += (unsigned long long)eb;
                my_fixed += (unsigned long long)fb;
                const uint32_t slot_of = ntok + (uint32_t)__popcll(T & low_mask(lane));
                if (slot_of < seg) tokens[slot_of] = word;
            }
            ntok += (uint32_t)__popcll(T);
        }
        const unsigned long long fixed_bits = 3ull + wave_sum(my_fixed) + 7ull, extra_bits = wave_sum(my_extra);
        if (lane == 0) hist[256] = 1u;
        __threadfence_block();   // the token words are read back by other lanes of this wave
        __syncthreads();

        // ---- build: the three codes and the size of the dynamic block
        for (int s = (int)lane; s < kPngLit; s += 64) sc.keys[s] = png_code_key(hist[s], (uint32_t)s);
        __syncthreads();
        wave_code_lengths(sc, kPngLit, 15, lens, lane);
        if (lane < (uint32_t)kPngDist) sc.keys[lane] = png_code_key(hist[kPngLit + lane], lane);
        __syncthreads();
        wave_code_lengths(sc, kPngDist, 15, lens + kPngLit, lane);
        if (lane == 0) {
            const int hlit = png_hlit(lens), hdist = png_hdist(lens + kPngLit);
            s_head[0] = hlit;
            s_head[1] = hdist;
            s_head[3] = png_cl_sequence(lens, hlit, lens + kPngLit, hdist, seq, cl_counts);
        }
        __syncthreads();
        if (lane < (uint32_t)kPngCl) sc.keys[lane] = png_code_key(cl_counts[lane], lane);
        __syncthreads();
        wave_code_lengths(sc, kPngCl, 7, lens + kPngLens, lane);
        if (lane == 0) s_head[2] = png_hclen(lens + kPngLens);
        __syncthreads();
        const int hlit = s_head[0], hdist = s_head[1], hclen = s_head[2], nseq = s_head[3];
        unsigned long long my_bits = 0;
        for (int k = (int)lane; k < nseq; k += 64) {   // <= 5
            const uint32_t sym = seq[k] & 31u;
            my_bits += (unsigned long long)lens[kPngLens + sym] + (unsigned long long)png_cl_extra(sym);
        }
        for (int s = (int)lane; s < kPngLens; s += 64) my_bits += (unsigned long long)hist[s] * lens[s];   // <= 5
        const unsigned long long dyn_bits = 3ull + 14ull + 3ull * (unsigned long long)hclen + extra_bits + wave_sum(my_bits);

        const uint32_t stored_bytes = png_stored_segment_bytes(n, last), fixed_bytes = png_huffman_segment_bytes(fixed_bits, last);
        const uint32_t dyn_bytes = png_huffman_segment_bytes(dyn_bits, last);
        const int type = png_segment_choice(stored_bytes, fixed_bytes, dyn_bytes);

        // ---- pass 2: the chosen type alone
        if (type == kPngStored) {
            if (lane == 0) {
                slot_b[0] = last ? 1 : 0;
                slot_b[1] = (uint8_t)(n & 0xFFu);
                slot_b[2] = (uint8_t)(n >> 8);
                slot_b[3] = (uint8_t)(~n & 0xFFu);
                slot_b[4] = (uint8_t)((~n >> 8) & 0xFFu);
                if (!last) {
                    slot_b[5u + n] = 0x00;
                    slot_b[6u + n] = 0x00;
                    slot_b[7u + n] = 0x00;
                    slot_b[8u + n] = 0xFF;
                    slot_b[9u + n] = 0xFF;
                }
            }
            for (uint32_t i = lane; i < n; i += 64u) slot_b[5u + i] = s_b[i];   // <= 512
        } else {
            const bool dyn = type == kPngDynamic;
            if (dyn && lane == 0) {
                png_canonical_codes(lens, kPngLit, codes);
                png_canonical_codes(lens + kPngLit, kPngDist, codes + kPngLit);
                png_canonical_codes(lens + kPngLens, kPngCl, codes + kPngLens);
            }
            for (uint32_t i = lane; i < (uint32_t)kDynStageWords; i += 64u) stage[i] = 0u;
            __syncthreads();
            if (lane == 0) stage[0] = (last ? 1u : 0u) | ((uint32_t)type << 1);   // BFINAL, BTYPE
            __syncthreads();

            unsigned long long bitpos = 3;   // of the block, from the slot's first bit (uniform)
            uint32_t stage_word = 0;         // the slot word stage[0] stands for (uniform)

            // ORs a token of <= 48 bits in at bit `where`, then moves the stage's whole words to the slot; `more` = the new bit position
            auto emit = [&](const unsigned long long bits, const int nb, const unsigned long long where, const unsigned long long more,
                            const bool all) {
                if (nb > 0) {
                    const uint32_t rel = (uint32_t)(where - 32ull * stage_word), wi = rel >> 5, sh = rel & 31u;   // wi <= 95
                    const unsigned long long lo = bits << sh;
                    atomicOr(&stage[wi], (uint32_t)lo);
                    if (lo >> 32) atomicOr(&stage[wi + 1u], (uint32_t)(lo >> 32));
                    const uint32_t hi = sh ? (uint32_t)(bits >> (64u - sh)) : 0u;
                    if (hi) atomicOr(&stage[wi + 2u], hi);
                }
                __syncthreads();
                uint32_t full = (uint32_t)(more >> 5) - stage_word;           // <= 96
                const uint32_t keep = all ? 0u : stage[full];                  // the word still being filled
                if (all && (more & 31ull)) ++full;
                const uint32_t mine0 = lane < full ? stage[lane] : 0u, mine1 = lane + 64u < full ? stage[lane + 64u] : 0u;
                __syncthreads();
                if (lane < full && stage_word + lane < slot_words) slot[stage_word + lane] = mine0;
                if (lane + 64u < full && stage_word + lane + 64u < slot_words) slot[stage_word + lane + 64u] = mine1;
                stage[lane] = lane == 0 ? keep : 0u;
                stage[lane + 64u] = 0u;
                __syncthreads();
                stage_word += full;
            };
            auto step = [&](const unsigned long long bits, const int nb) {   // one token a lane, in lane order
                const uint32_t incl = wave_incl_sum((uint32_t)nb, lane);
                const uint32_t step_bits = __shfl(incl, 63);
                emit(bits, nb, bitpos + incl - (uint32_t)nb, bitpos + step_bits, false);
                bitpos += step_bits;
            };

            if (dyn) {
                unsigned long long hb = 0;
                int hn = 0;
                if (lane == 0) {
                    hb = (unsigned long long)(hlit - 257) | ((unsigned long long)(hdist - 1) << 5) | ((unsigned long long)(hclen - 4) << 10);
                    hn = 14;
                } else if (lane <= (uint32_t)hclen) {
                    hb = lens[kPngLens + png_cl_order((int)lane - 1)];
                    hn = 3;
                }
                step(hb, hn);
                for (int base = 0; base < nseq; base += 64) {   // <= 5
                    PngBits t;
                    t.bits = 0u;
                    t.nb = 0;
                    if (base + (int)lane < nseq) t = png_cl_entry(seq[base + (int)lane], codes + kPngLens);
                    step(t.bits, t.nb);
                }
            }
            for (uint32_t base = 0; base < ntok; base += 64u) {   // <= 512
                unsigned long long tb = 0;
                int tn = 0;
                if (base + lane < ntok && base + lane < seg) {
                    const uint32_t word = tokens[base + lane];
                    if (dyn) {
                        const PngBits64 t = png_dynamic_token(word, codes, codes + kPngLit);
                        tb = t.bits;
                        tn = t.nb;
                    } else {
                        const PngBits t = png_fixed_token(word);
                        tb = t.bits;
                        tn = t.nb;
                    }
                }
                step(tb, tn);
            }
            step(dyn ? (unsigned long long)(codes[256] & 0xFFFFu) : 0ull, lane == 0 ? (dyn ? (int)(codes[256] >> 16) : 7) : 0);   // end of block
            if (!last) {
                const unsigned long long aligned = (bitpos + 3ull + 7ull) & ~7ull;
                emit(0xFFFF0000ull, lane == 0 ? 32 : 0, aligned, aligned + 32ull, true);   // 00 00 FF FF
            } else {
                emit(0ull, 0, bitpos, bitpos, true);
            }
        }
        if (lane == 0) {
            SegRec r;
            r.len = type == kPngStored ? stored_bytes : type == kPngFixed ? fixed_bytes : dyn_bytes;
            r.s1 = (uint32_t)(s1 % kAdlerMod);
            r.s2 = (uint32_t)(s2 % kAdlerMod);
            r.off = 0u;
            rec[id] = r;
        }
    }
}

struct PngPlan {
    long long F, seg, slot_bytes, total_segs;
    int n_seg;
    size_t slots_off, total;
};

size_t round16(const size_t v) { return (v + 15u) & ~(size_t)15u; }

// png_geometry_ok(h, w, depth, seg_bytes), n_frames >= 0 (the callers check)
PngPlan png_plan(const int n_frames, const int h, const int w, const int depth, const int seg_bytes)
{
    PngPlan p;
    p.F = png_filtered_size(h, w, depth);
    p.seg = seg_bytes < p.F ? seg_bytes : p.F;
    p.n_seg = (int)png_segments(p.F, seg_bytes);
    p.total_segs = (long long)p.n_seg * (long long)n_frames;
    p.slot_bytes = 4 * ((p.seg + 10 + 3) / 4) + 4;   // a stored segment and its realigning block, in whole words, and one to spare
    p.slots_off = round16((size_t)p.total_segs * sizeof(SegRec));
    p.total = p.slots_off + (size_t)p.total_segs * (size_t)p.slot_bytes;
    return p;
}

int launch_png_deflate(const uint8_t *planes, int n_frames, int h, int w, int depth, const PngPlan &p, uint8_t *out, long long out_stride,
                       long long *sizes, uint8_t *ws, hipStream_t s)
{
    SegRec *rec = reinterpret_cast<SegRec *>(ws);
    uint8_t *slots = ws + p.slots_off;
    const int total = (int)p.total_segs;
    const int grid = total < kSegMaxBlocks ? total : kSegMaxBlocks;
    hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)grid), dim3(64), 0, s, planes, h, w, depth, png_row_bytes(w, depth), (uint32_t)p.F,
                       (uint32_t)p.seg, p.n_seg, total, slots, p.slot_bytes, rec);
    DP_HIP(hipGetLastError());
    hipLaunchKernelGGL(png_layout_kernel, dim3((unsigned)n_frames), dim3(64), 0, s, rec, p.n_seg, (uint32_t)p.F, (uint32_t)p.seg, out, out_stride, sizes);
    DP_HIP(hipGetLastError());
    const int bpf = p.n_seg < kPackMaxBlocksPerFrame ? p.n_seg : kPackMaxBlocksPerFrame;
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)bpf, (unsigned)n_frames), dim3(kPackThreads), 0, s, (const SegRec *)rec, p.n_seg,
                       (const uint8_t *)slots, p.slot_bytes, out, out_stride);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

// the plan of the fixed-mode call, and behind its slots the token area: seg 32-bit words per segment
struct PngDynWorkspace {
    PngPlan base;
    size_t tokens_off, total;
};

PngDynWorkspace png_dyn_plan(const int n_frames, const int h, const int w, const int depth, const int seg_bytes)
{
    PngDynWorkspace p;
    p.base = png_plan(n_frames, h, w, depth, seg_bytes);
    p.tokens_off = round16(p.base.total);
    p.total = p.tokens_off + (size_t)p.base.total_segs * (size_t)p.base.seg * sizeof(uint32_t);
    return p;
}

int launch_png_deflate_dyn(const uint8_t *planes, int n_frames, int h, int w, int depth, const PngDynWorkspace &d, uint8_t *out, long long out_stride,
                           long long *sizes, uint8_t *ws, hipStream_t s)
{
    const PngPlan &p = d.base;
    SegRec *rec = reinterpret_cast<SegRec *>(ws);
    uint8_t *slots = ws + p.slots_off;
    uint32_t *tokens = reinterpret_cast<uint32_t *>(ws + d.tokens_off);
    const int total = (int)p.total_segs;
    const int grid = total < kSegMaxBlocks ? total : kSegMaxBlocks;
    hipLaunchKernelGGL(png_segment_dyn_kernel, dim3((unsigned)grid), dim3(64), 0, s, planes, h, w, depth, png_row_bytes(w, depth), (uint32_t)p.F,
                       (uint32_t)p.seg, p.n_seg, total, slots, p.slot_bytes, tokens, rec);
    DP_HIP(hipGetLastError());
    hipLaunchKernelGGL(png_layout_kernel, dim3((unsigned)n_frames), dim3(64), 0, s, rec, p.n_seg, (uint32_t)p.F, (uint32_t)p.seg, out, out_stride, sizes);
    DP_HIP(hipGetLastError());
    const int bpf = p.n_seg < kPackMaxBlocksPerFrame ? p.n_seg : kPackMaxBlocksPerFrame;
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)bpf, (unsigned)n_frames), dim3(kPackThreads), 0, s, (const SegRec *)rec, p.n_seg,
                       (const uint8_t *)slots, p.slot_bytes, out, out_stride);
    DP_HIP(hipGetLastError());
    return DP_OK;
}

int check_png(const char *fn, const void *planes, int n_frames, int h, int w, int depth, int seg_bytes, const void *out, int64_t out_stride,
              const void *sizes)
{
    if (!planes || !out || !sizes || n_frames < 0 || !png_geometry_ok(h, w, depth, seg_bytes)) {
        set_error("%s: bad argument (h, w >= 1, depth in {1, 2, 4, 8}, seg_bytes in 256 ... 32768, filtered bytes < 2^31, n_frames >= 0)", fn);
        return DP_EINVAL;
    }
    const uint64_t need = png_deflate_bound(png_filtered_size(h, w, depth), seg_bytes);
    if (out_stride < 0 || (uint64_t)out_stride < need) {
        set_error("%s: bad argument (out_stride of %lld bytes is below the bound of %llu for %d x %d at depth %d, seg_bytes %d)", fn,
                  (long long)out_stride, (unsigned long long)need, h, w, depth, seg_bytes);
        return DP_EINVAL;
    }
    return DP_OK;
}

int check_code_lengths(const char *fn, const void *counts, int n_alphabets, int n_symbols, int max_len, const void *lengths)
{
    if (!counts || !lengths || n_alphabets < 0 || n_symbols < 2 || n_symbols > kPngLit || max_len < 1 || max_len > 15 ||
        (1 << max_len) < n_symbols || ((uintptr_t)counts & 3)) {
        set_error("%s: bad argument (n_alphabets >= 0, n_symbols in 2 ... 286, max_len in 1 ... 15 with 2^max_len >= n_symbols, counts 4-byte aligned)", fn);
        return DP_EINVAL;
    }
    return DP_OK;
}

}  // namespace
}  // namespace dp

using namespace dp;

extern "C" {

size_t dp_png_filtered_bytes(int h, int w, int depth)
{
    if (!png_geometry_ok(h, w, depth, kPngSegMin)) return 0;
    return (size_t)png_filtered_size(h, w, depth);
}

size_t dp_png_deflate_bound_bytes(int h, int w, int depth, int seg_bytes)
{
    if (!png_geometry_ok(h, w, depth, seg_bytes)) return 0;
    return (size_t)png_deflate_bound(png_filtered_size(h, w, depth), seg_bytes);
}

size_t dp_png_deflate_workspace_bytes(int n_frames, int h, int w, int depth, int seg_bytes)
{
    if (!png_geometry_ok(h, w, depth, seg_bytes) || n_frames < 0) return 0;
    return png_plan(n_frames, h, w, depth, seg_bytes).total;
}

int dp_png_deflate_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_dev,
                             int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream)
{
    const char *fn = "dp_png_deflate_encode_u8";
    try {
        const int rc = check_png(fn, planes_dev, n_frames, h, w, depth, seg_bytes, out_dev, out_stride, sizes_dev);
        if (rc != DP_OK) return rc;
        if (!ws_dev || ((uintptr_t)ws_dev & 15) || ((uintptr_t)sizes_dev & 7)) {
            set_error("%s: bad argument (ws_dev 16-byte, sizes_dev 8-byte aligned)", fn);
            return DP_EINVAL;
        }
        if (n_frames > 65535) {
            set_error("%s: at most 65535 frames per call, not %d", fn, n_frames);
            return DP_EUNSUPPORTED;
        }
        const PngPlan p = png_plan(n_frames, h, w, depth, seg_bytes);
        if (p.total_segs >= (1LL << 31)) {
            set_error("%s: %d frames of %d segments are 2^31 segments or more: cut the batch or raise seg_bytes", fn, n_frames, p.n_seg);
            return DP_EUNSUPPORTED;
        }
        if (ws_bytes < p.total) {
            set_error("%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, p.total);
            return DP_EWORKSPACE;
        }
        if (n_frames == 0) return DP_OK;
        return launch_png_deflate(planes_dev, n_frames, h, w, depth, p, out_dev, (long long)out_stride, reinterpret_cast<long long *>(sizes_dev),
                                  static_cast<uint8_t *>(ws_dev), (hipStream_t)stream);
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
}

int dp_png_deflate_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_host,
                           int64_t out_stride, int64_t *sizes_host)
{
    const char *fn = "dp_png_deflate_host_u8";
    try {
        const int rc = check_png(fn, planes_host, n_frames, h, w, depth, seg_bytes, out_host, out_stride, sizes_host);
        if (rc != DP_OK) return rc;
        const size_t n_px = (size_t)h * (size_t)w;
        std::vector<uint8_t> frame;
        for (int f = 0; f < n_frames; ++f) {
            png_deflate_encode(planes_host + (size_t)f * n_px, h, w, depth, seg_bytes, frame);
            if ((int64_t)frame.size() > out_stride) {   // (the bound says it cannot be)
                set_error("%s: frame %d of %zu bytes exceeds the stride", fn, f, frame.size());
                return DP_EINVAL;
            }
            std::copy(frame.begin(), frame.end(), out_host + (size_t)f * (size_t)out_stride);
            sizes_host[f] = (int64_t)frame.size();
        }
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
    return DP_OK;
}

size_t dp_png_deflate_dyn_workspace_bytes(int n_frames, int h, int w, int depth, int seg_bytes)
{
    if (!png_geometry_ok(h, w, depth, seg_bytes) || n_frames < 0) return 0;
    if (n_frames == 0) return 0;
    return png_dyn_plan(n_frames, h, w, depth, seg_bytes).total;
}

int dp_png_deflate_dyn_encode_u8(const uint8_t *planes_dev, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_dev,
                                 int64_t out_stride, int64_t *sizes_dev, void *ws_dev, size_t ws_bytes, void *stream)
{
    const char *fn = "dp_png_deflate_dyn_encode_u8";
    try {
        const int rc = check_png(fn, planes_dev, n_frames, h, w, depth, seg_bytes, out_dev, out_stride, sizes_dev);
        if (rc != DP_OK) return rc;
        if (!ws_dev || ((uintptr_t)ws_dev & 15) || ((uintptr_t)sizes_dev & 7)) {
            set_error("%s: bad argument (ws_dev 16-byte, sizes_dev 8-byte aligned)", fn);
            return DP_EINVAL;
        }
        if (n_frames > 65535) {
            set_error("%s: at most 65535 frames per call, not %d", fn, n_frames);
            return DP_EUNSUPPORTED;
        }
        const PngDynWorkspace p = png_dyn_plan(n_frames, h, w, depth, seg_bytes);
        if (p.base.total_segs >= (1LL << 31)) {
            set_error("%s: %d frames of %d segments are 2^31 segments or more: cut the batch or raise seg_bytes", fn, n_frames, p.base.n_seg);
            return DP_EUNSUPPORTED;
        }
        if (n_frames == 0) return DP_OK;
        if (ws_bytes < p.total) {
            set_error("%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, p.total);
            return DP_EWORKSPACE;
        }
        return launch_png_deflate_dyn(planes_dev, n_frames, h, w, depth, p, out_dev, (long long)out_stride, reinterpret_cast<long long *>(sizes_dev),
                                      static_cast<uint8_t *>(ws_dev), (hipStream_t)stream);
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
}

int dp_png_deflate_dyn_host_u8(const uint8_t *planes_host, int n_frames, int h, int w, int depth, int seg_bytes, uint8_t *out_host,
                               int64_t out_stride, int64_t *sizes_host)
{
    const char *fn = "dp_png_deflate_dyn_host_u8";
    try {
        const int rc = check_png(fn, planes_host, n_frames, h, w, depth, seg_bytes, out_host, out_stride, sizes_host);
        if (rc != DP_OK) return rc;
        const size_t n_px = (size_t)h * (size_t)w;
        std::vector<uint8_t> frame;
        for (int f = 0; f < n_frames; ++f) {
            png_deflate_encode_dyn(planes_host + (size_t)f * n_px, h, w, depth, seg_bytes, frame);
            if ((int64_t)frame.size() > out_stride) {   // (the bound says it cannot be)
                set_error("%s: frame %d of %zu bytes exceeds the stride", fn, f, frame.size());
                return DP_EINVAL;
            }
            std::copy(frame.begin(), frame.end(), out_host + (size_t)f * (size_t)out_stride);
            sizes_host[f] = (int64_t)frame.size();
        }
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
    return DP_OK;
}

int dp_png_code_lengths_u8(const uint32_t *counts_dev, int n_alphabets, int n_symbols, int max_len, uint8_t *lengths_dev, void *stream)
{
    const char *fn = "dp_png_code_lengths_u8";
    try {
        const int rc = check_code_lengths(fn, counts_dev, n_alphabets, n_symbols, max_len, lengths_dev);
        if (rc != DP_OK) return rc;
        if (n_alphabets == 0) return DP_OK;
        const int grid = n_alphabets < kSegMaxBlocks ? n_alphabets : kSegMaxBlocks;
        hipLaunchKernelGGL(png_code_lengths_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, counts_dev, n_alphabets, n_symbols,
                           max_len, lengths_dev);
        DP_HIP(hipGetLastError());
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
    return DP_OK;
}

int dp_png_code_lengths_host(const uint32_t *counts_host, int n_alphabets, int n_symbols, int max_len, uint8_t *lengths_host)
{
    const char *fn = "dp_png_code_lengths_host";
    try {
        const int rc = check_code_lengths(fn, counts_host, n_alphabets, n_symbols, max_len, lengths_host);
        if (rc != DP_OK) return rc;
        for (size_t i = 0; i < (size_t)n_alphabets * (size_t)n_symbols; ++i)
            if (counts_host[i] > kPngMaxCount) {
                set_error("%s: bad argument (count %u of symbol %zu is above 2^20)", fn, counts_host[i], i);
                return DP_EINVAL;
            }
        PngCodeScratch sc;
        for (int a = 0; a < n_alphabets; ++a)
            png_code_lengths(counts_host + (size_t)a * (size_t)n_symbols, n_symbols, max_len, lengths_host + (size_t)a * (size_t)n_symbols, sc);
    } catch (const std::exception &e) {
        set_error("%s: %s", fn, e.what());
        return DP_ENOMEM;
    } catch (...) {
        set_error("%s: unexpected exception", fn);
        return DP_ENOMEM;
    }
    return DP_OK;
}

}  // extern "C"
