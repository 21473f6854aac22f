// entropy_motion_kernels.hip -- the entropy coder of the motion stream (xEntropyEncodeMvGpu, xEntropyDecodeMvGpu) and the vectors from the
// differences (xMotionReconstructGpu).  The contract is include/x266hip.h's; the syntax of a CTU is x266_entropy_motion.hpp's and the coder
// x266_entropy.hpp's -- the very functions the host helpers run --, geometry, mask test and predictor x266_motion.hpp's.
//
// The coder has the shape of entropy_kernels.hip: one wave per CTU, four waves a workgroup.  Lanes bring the CTU's at most 512 payload bytes
// into LDS and test the mask as motion_unpack_kernel does, lane 0 runs the coder's chain over LDS with the 7 contexts there, and the bytes
// cross an LDS slab at the stream's own 16-byte phase with the level coder's copy (substream_copy).  Encode is count, the level stream's
// offset scan on this record, write; decode is one launch, CTU c's payload at the fixed place 256 c.
// Reconstruct walks the frame as a wavefront: a CTU's predictors read the CTUs to its left, above, above left and above right, so CTU
// (cx, cy) belongs to step cx + 2 cy; one launch per step on the caller's stream, ordered by the stream alone.
// No atomics, no allocation, no workgroup waits for another: the bytes depend on the data alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_entropy.hpp"
#include "x266_entropy_motion.hpp"
#include "x266_lanes.hpp"
#include "x266_levels.hpp"
#include "x266_motion.hpp"

namespace x266 {
namespace {

constexpr unsigned kEntropyWavesPerWg = 4;

// ---- the coder: pack's records and words <-> one record and one substream per CTU ---------------------------------------------------------
constexpr unsigned kMotionStreamSlabBytes = kEntropyMotionMaxBytes + 16;
constexpr unsigned kMotionCtxSlab = 8;                                      // 7 contexts
static_assert(kMotionStreamSlabBytes % 16 == 0, "slabs hold whole 16-byte chunks");
static_assert(sizeof(x266_entropy_motion_ctu_t) == 32 && offsetof(x266_entropy_motion_ctu_t, offset) == offsetof(x266_level_region_t, offset) &&
                  offsetof(x266_entropy_motion_ctu_t, n_words) == offsetof(x266_level_region_t, n_words),
              "the offset scan reads n_words and writes offset where the level record has them");

// WRITE false: the count step, every field of the record but `offset`.  WRITE true: the write step, after the scan.
template <bool WRITE>
__global__ __launch_bounds__(64 * kEntropyWavesPerWg) void entropy_motion_encode_kernel(const x266_motion_ctu_t *__restrict__ ctu, const uint16_t *__restrict__ words,
                                                                                       x266_entropy_motion_ctu_t *coded, uint16_t *__restrict__ stream, int bw, int bh,
                                                                                       size_t n_ctu, uint64_t in_words, uint64_t cap_words, const EntropyMotionInit init)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds_words[kEntropyWavesPerWg][kMotionCtuWords];
    __shared__ __attribute__((aligned(16))) char lds_stream[WRITE ? kEntropyWavesPerWg : 1][WRITE ? kMotionStreamSlabBytes : 16];
    __shared__ uint16_t lds_ctx[kEntropyWavesPerWg][kMotionCtxSlab];
    __shared__ uint32_t lds_bytes[kEntropyWavesPerWg];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t c = (size_t)blockIdx.x * kEntropyWavesPerWg + wave_in_wg;
    const bool active = c < n_ctu;
    uint64_t head_mask = 0, in_offset = 0;
    if (active) {
        head_mask = ctu[c].head_mask;
        in_offset = ctu[c].offset;
    }
    const MotionCtu g = motion_ctu(bw, bh, active ? c : 0);
    const uint64_t exist_mask = __ballot(motion_block_exists(g, lane));
    const uint64_t uncovered = __ballot(!motion_block_covered(g, head_mask, lane));
    const unsigned parts = (unsigned)__popcll(head_mask);
    const uint64_t n_in = (uint64_t)kMotionWordsPerPart * parts;            // at most 256: no sum below can wrap
    const bool readable = active && motion_mask_plausible(head_mask, exist_mask) && uncovered == 0 && in_offset <= in_words && n_in <= in_words - in_offset;
    bool skip = !readable;                                                 // wave-uniform: no word of the CTU is read
    uint64_t offset = 0;
    uint32_t n_words = 0;
    if (WRITE && active) {
        n_words = coded[c].n_words;
        offset = coded[c].offset;
        if (n_words == 0 || offset > cap_words || n_words > cap_words - offset) skip = true;
    }
    uint16_t *own = lds_words[wave_in_wg];
    uint16_t *ctx = lds_ctx[wave_in_wg];
    if (!skip && lane < parts) {                                            // 16-bit loads: an offset from a host has no alignment
        const uint16_t *at = words + in_offset + (size_t)kMotionWordsPerPart * lane;
        uint2 w;
        w.x = (uint32_t)at[0] | (uint32_t)at[1] << 16;
        w.y = (uint32_t)at[2] | (uint32_t)at[3] << 16;
        *reinterpret_cast<uint2 *>(own + kMotionWordsPerPart * lane) = w;
    }
    if (lane < kEntropyMotionContexts) ctx[lane] = init.p[lane];
    __syncthreads();
    const unsigned phase = (unsigned)(offset & 7u);
    uint8_t *pay = reinterpret_cast<uint8_t *>(lds_stream[WRITE ? wave_in_wg : 0]) + phase * 2;
    if (lane == 0 && active && (!WRITE || !skip)) {                         // the serial section: the coder's state is one chain
        EntropyEnc e;
        entropy_enc_start(e, WRITE ? pay : nullptr, WRITE ? kEntropyMotionMaxBytes : 0u);
        if (readable) entropy_motion_encode_ctu(e, g, head_mask, own, ctx);
        const uint32_t n_bytes = entropy_enc_finish(e);                     // an unreadable CTU codes no bin: no bytes
        if (WRITE) {
            if (n_bytes <= kEntropyMotionMaxBytes && (n_bytes & 1u)) pay[n_bytes] = 0;      // the pad byte
            lds_bytes[wave_in_wg] = n_bytes;
        } else {
            x266_entropy_motion_ctu_t *rec = coded + c;
            rec->ctx_bins = e.ctx_bins;
            rec->bypass_bins = e.bypass_bins;
            rec->n_words = (n_bytes + 1u) >> 1;
            rec->n_bytes = n_bytes;
            rec->parts = readable ? parts : 0u;
            rec->unreadable = readable ? 0u : 1u;
        }
    }
    if (!WRITE) return;
    __syncthreads();
    if (skip) return;
    const uint32_t n_bytes = lds_bytes[wave_in_wg];
    if (n_bytes > kEntropyMotionMaxBytes || ((n_bytes + 1u) >> 1) != n_words) return;      // as counted; held against the record all the same
    substream_copy(stream + (offset - phase), reinterpret_cast<const uint16_t *>(lds_stream[wave_in_wg]), phase, n_words, lane);
}

__global__ __launch_bounds__(64 * kEntropyWavesPerWg) void entropy_motion_decode_kernel(x266_motion_ctu_t *__restrict__ ctu, uint16_t *__restrict__ words,
                                                                                       const x266_entropy_motion_ctu_t *__restrict__ coded,
                                                                                       const uint16_t *__restrict__ stream, uint8_t *__restrict__ status, int bw, int bh,
                                                                                       size_t n_ctu, uint64_t cap_words, const EntropyMotionInit init)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds_words[kEntropyWavesPerWg][kMotionCtuWords];
    __shared__ __attribute__((aligned(16))) char lds_stream[kEntropyWavesPerWg][kMotionStreamSlabBytes];
    __shared__ uint16_t lds_ctx[kEntropyWavesPerWg][kMotionCtxSlab];
    __shared__ EntropyMotionCtu lds_out[kEntropyWavesPerWg];
    __shared__ uint32_t lds_status[kEntropyWavesPerWg];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t c = (size_t)blockIdx.x * kEntropyWavesPerWg + wave_in_wg;
    const bool active = c < n_ctu;
    uint64_t offset = 0;
    uint32_t n_bytes = 0;
    if (active) {
        offset = coded[c].offset;
        n_bytes = coded[c].n_bytes;
    }
    uint32_t n_words = (n_bytes >> 1) + (n_bytes & 1u);                      // no wrap at 2^32 - 1
    const bool ok = active && n_bytes <= kEntropyMotionMaxBytes && offset <= cap_words && n_words <= cap_words - offset;
    if (!ok) {                                                              // the empty substream
        offset = 0;
        n_bytes = n_words = 0;
    }
    const unsigned phase = (unsigned)(offset & 7u);
    uint16_t *pay = reinterpret_cast<uint16_t *>(lds_stream[wave_in_wg]);
    if (n_words) substream_copy(pay, stream + (offset - phase), phase, n_words, lane);
    uint16_t *own = lds_words[wave_in_wg];
    uint16_t *ctx = lds_ctx[wave_in_wg];
    if (lane < kEntropyMotionContexts) ctx[lane] = init.p[lane];
    __syncthreads();
    const MotionCtu g = motion_ctu(bw, bh, active ? c : 0);
    if (lane == 0 && active) {                                              // the serial section
        EntropyDec d;
        entropy_dec_start(d, reinterpret_cast<const uint8_t *>(pay + phase), n_bytes);
        EntropyMotionCtu r;
        uint32_t st = ok ? 0u : 1u;
        if (!entropy_motion_decode_ctu(d, g, ctx, own, &r)) {
            entropy_motion_flat_ctu(g, ctx, own, &r);
            st = 2u;
        }
        lds_out[wave_in_wg] = r;
        lds_status[wave_in_wg] = st;
    }
    __syncthreads();
    if (!active) return;
    const EntropyMotionCtu r = lds_out[wave_in_wg];
    uint16_t *dst = words + c * kMotionCtuWords;                            // 512-byte aligned: d_words is 16-byte aligned
    if (lane < r.parts) *reinterpret_cast<uint2 *>(dst + kMotionWordsPerPart * lane) = *reinterpret_cast<const uint2 *>(own + kMotionWordsPerPart * lane);
    if (lane == 0) {
        x266_motion_ctu_t *rec = ctu + c;
        rec->head_mask = r.mask;
        rec->offset = (uint64_t)c * kMotionCtuWords;
        rec->n_words = (uint32_t)kMotionWordsPerPart * r.parts;
        rec->parts = r.parts;
        rec->bits = r.bits;
        rec->max_abs = r.max_abs;
        if (status) status[c] = (uint8_t)lds_status[wave_in_wg];
    }
}

EntropyMotionInit entropy_motion_table(const uint16_t *init)
{
    EntropyMotionInit t = kEntropyMotionDefault;
    if (init)
        for (unsigned i = 0; i < kEntropyMotionContexts; ++i) t.p[i] = init[i];
    return t;
}

// ---- the vectors from the differences ------------------------------------------------------------------------------------------------------
// xMotionReconstructGpu, one step of the wavefront: the CTUs (step - 2 cy, cy), cy = cy_first + blockIdx.x, one wave (one workgroup) each.
// Everything a predictor of this CTU can ask for lies in a 10 x 9 grid of vectors in LDS: the CTU's own 8 x 8 blocks at (1.., 1..), the
// row above from the block above left to the first block of the CTU above right at (0..9, 0), the column to the left at (0, 1..8).  The
// border comes from d_mv, which the launches of earlier steps wrote; the own blocks are written as the chain decides them and read from
// there -- never back through global memory.  The chain is a wave-uniform loop over the heads of the mask; every lane computes the same
// predictor from broadcast LDS reads, the lanes of the partition store the vector, and a barrier (a wave's own: the workgroup is one
// wave) orders the store before the next partition's reads.
constexpr unsigned kReconGridW = 10, kReconGridH = 9;

__global__ __launch_bounds__(64) void motion_reconstruct_kernel(x266_me_result_t *mv, uint8_t *__restrict__ level, const x266_motion_ctu_t *__restrict__ ctu,
                                                                const uint16_t *__restrict__ stream, int bw, int bh, int cw, int step, int cy_first,
                                                                uint64_t cap_words)
{
    __shared__ uint32_t grid[kReconGridW * kReconGridH];                    // mvx | mvy << 16
    __shared__ uint32_t diff[64];                                           // words 2 and 3 of partition j
    const unsigned lane = threadIdx.x;
    const int cy = cy_first + (int)blockIdx.x, cx = step - 2 * cy;          // inside the frame: the launch counts them
    const size_t c = (size_t)cy * (size_t)cw + (size_t)cx;
    const uint64_t m = ctu[c].head_mask, offset = ctu[c].offset;
    const uint64_t head_mask = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32;
    const MotionCtu g = motion_ctu(bw, bh, c);
    const bool exists = motion_block_exists(g, lane);
    const uint64_t exist_mask = __ballot(exists);
    const uint64_t uncovered = __ballot(!motion_block_covered(g, head_mask, lane));
    const unsigned parts = (unsigned)__popcll(head_mask);
    const uint64_t n_words = (uint64_t)kMotionWordsPerPart * parts;         // at most 256: no sum below can wrap
    const bool ok = motion_mask_plausible(head_mask, exist_mask) && uncovered == 0 && offset <= cap_words && n_words <= cap_words - offset;
    const unsigned own_at = (motion_morton_y(lane) + 1u) * kReconGridW + motion_morton_x(lane) + 1u;
    uint2 rec = {0u, 0u};                                                   // mvx | mvy << 16, cost = 0
    uint8_t lvl = 0;
    if (ok) {                                                               // wave-uniform
        if (lane < kReconGridW + 8u) {
            const int lx = lane < kReconGridW ? (int)lane - 1 : -1, ly = lane < kReconGridW ? -1 : (int)lane - (int)kReconGridW;
            const int bx = g.X0 + lx, by = g.Y0 + ly;
            uint32_t v = 0;                                                 // a spot outside the frame is never asked for
            if (bx >= 0 && bx < bw && by >= 0 && by < bh) v = reinterpret_cast<const uint32_t *>(mv + ((size_t)by * (size_t)bw + (size_t)bx))[0];
            grid[(unsigned)(ly + 1) * kReconGridW + (unsigned)(lx + 1)] = v;
        }
        if (lane < parts) {                                                 // 16-bit loads: an offset from a host decoder has no alignment
            const uint16_t *at = stream + offset + (size_t)kMotionWordsPerPart * lane + 2;
            diff[lane] = (uint32_t)at[0] | (uint32_t)at[1] << 16;
        }
        __syncthreads();
        unsigned j = 0;
        for (uint64_t left = head_mask; left; left &= left - 1u, ++j) {
            const unsigned h = (unsigned)__builtin_ctzll(left);
            const int k = motion_head_level(g, head_mask, h), X = motion_block_x(g, h), Y = motion_block_y(g, h);
            const PartVec p = motion_predictor_from(
                [&](int bx, int by) {
                    const uint32_t v = grid[(unsigned)(by - g.Y0 + 1) * kReconGridW + (unsigned)(bx - g.X0 + 1)];
                    return PartVec{(int16_t)(v & 0xFFFFu), (int16_t)(v >> 16)};
                },
                bw, X, Y, 1 << k);
            const uint32_t d = diff[j];
            const uint32_t qx = (uint32_t)(p.x + (int16_t)(d & 0xFFFFu)) & 0xFFFFu, qy = (uint32_t)(p.y + (int16_t)(d >> 16)) & 0xFFFFu;
            if (motion_node_first(lane, k) == h) grid[own_at] = qx | qy << 16;
            __syncthreads();
        }
        rec.x = grid[own_at];
        lvl = (uint8_t)motion_head_level(g, head_mask, (unsigned)motion_head_of(head_mask, lane));
    }
    if (!exists) return;
    const size_t b = (size_t)motion_block_y(g, lane) * (size_t)bw + (size_t)motion_block_x(g, lane);
    *reinterpret_cast<uint2 *>(mv + b) = rec;
    level[b] = lvl;
}

}  // namespace

hipError_t launch_entropy_motion_encode(const x266_entropy_motion_t &p, hipStream_t stream)
{
    const int bw = p.width / 8, bh = p.height / 8;
    const size_t n_ctu = (size_t)motion_ctus_w(bw) * (size_t)motion_ctus_h(bh);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(n_ctu, kEntropyWavesPerWg, &wgs)) return e;
    const dim3 block(64 * kEntropyWavesPerWg);
    const EntropyMotionInit init = entropy_motion_table(p.init);
    hipLaunchKernelGGL(entropy_motion_encode_kernel<false>, dim3(wgs), block, 0, stream, (const x266_motion_ctu_t *)p.d_ctu, (const uint16_t *)p.d_words, p.d_coded,
                       (uint16_t *)nullptr, bw, bh, n_ctu, p.in_words, (uint64_t)0, init);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(levels_scan_kernel<x266_entropy_motion_ctu_t>, dim3(1), dim3(kLevelsScanChunk), 0, stream, p.d_coded, n_ctu, p.cap_words, p.d_total);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.cap_words && p.d_stream)
        hipLaunchKernelGGL(entropy_motion_encode_kernel<true>, dim3(wgs), block, 0, stream, (const x266_motion_ctu_t *)p.d_ctu, (const uint16_t *)p.d_words, p.d_coded,
                           p.d_stream, bw, bh, n_ctu, p.in_words, p.cap_words, init);
    return hipGetLastError();
}

hipError_t launch_entropy_motion_decode(const x266_entropy_motion_t &p, hipStream_t stream)
{
    const int bw = p.width / 8, bh = p.height / 8;
    const size_t n_ctu = (size_t)motion_ctus_w(bw) * (size_t)motion_ctus_h(bh);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(n_ctu, kEntropyWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(entropy_motion_decode_kernel, dim3(wgs), dim3(64 * kEntropyWavesPerWg), 0, stream, p.d_ctu, p.d_words,
                       (const x266_entropy_motion_ctu_t *)p.d_coded, (const uint16_t *)p.d_stream, p.d_status, bw, bh, n_ctu, p.cap_words, entropy_motion_table(p.init));
    return hipGetLastError();
}

hipError_t launch_motion_reconstruct(const x266_motion_t &p, hipStream_t stream)
{
    const int bw = p.width / 8, bh = p.height / 8, cw = motion_ctus_w(bw), ch = motion_ctus_h(bh);
    const long steps = (long)cw + 2L * (ch - 1);
    for (long s = 0; s < steps; ++s) {                                      // CTU (cx, cy) with cx + 2 cy == s and 0 <= cx < cw
        const long lo = s - (cw - 1) > 0 ? (s - (cw - 1) + 1) / 2 : 0, hi = s / 2 < ch - 1 ? s / 2 : ch - 1;
        if (lo > hi) continue;                                              // a frame one CTU wide has no CTU on its odd steps
        hipLaunchKernelGGL(motion_reconstruct_kernel, dim3((unsigned)(hi - lo + 1)), dim3(64), 0, stream, p.d_mv, p.d_level, (const x266_motion_ctu_t *)p.d_ctu,
                           (const uint16_t *)p.d_stream, bw, bh, cw, (int)s, (int)lo, p.cap_words);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace x266
