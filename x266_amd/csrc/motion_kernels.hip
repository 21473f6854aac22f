// motion_kernels.hip -- the compact motion stream (xMotionPackGpu, xMotionUnpackGpu): the decided field of xInterPartitionDecideGpu, one
// record per 8x8 block and a level byte beside it, <-> one 32-byte record per CTU and four 16-bit words per partition in coding order.
// The contract is include/x266hip.h's, the Morton map, the walk, the level-from-mask rule, the well-formedness test and the causal
// predictor x266_motion.hpp's (the host helpers run the same functions), the geometry and the median x266_part.hpp's.
//
// One wave per CTU, lane = Morton block.  A lane reads its own level byte and takes the bytes of the first blocks of its three nodes from
// their lanes; the first whole node from level 3 down whose first block says "at least this level" is its partition, __ballot of the
// lanes that are first blocks is head_mask, and the popcount of the mask below a head is its place in the payload.  Only head lanes read
// vectors: their own and the three spots of the causal predictor, straight from d_mv (the wave has the lines in cache).
// Pack is three launches on one stream, as the level stream's: count (records without offsets), the offset scan (x266_levels.hpp's kernel
// on this record, whose first 20 bytes are the level record's), write (each head lane stores its 8 bytes; offsets are multiples of four
// words, so every store is aligned).  Unpack is one launch: the mask is tested lane by lane before any word of the stream is read.
// No atomics, no workgroup waits for another: the bytes depend on the data alone.
// xMotionReconstructGpu, unpack for a stream that carries only the differences, is entropy_motion_kernels.hip's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_levels.hpp"
#include "x266_motion.hpp"

namespace x266 {
namespace {

constexpr unsigned kMotionWavesPerWg = 4;
static_assert(sizeof(x266_motion_ctu_t) == 32 && sizeof(x266_level_region_t) == 32, "the records are 32 bytes");
static_assert(offsetof(x266_motion_ctu_t, offset) == offsetof(x266_level_region_t, offset) &&
                  offsetof(x266_motion_ctu_t, n_words) == offsetof(x266_level_region_t, n_words),
              "the offset scan reads n_words and writes offset where the level record has them");

// WRITE false: the count step, every field of the record but `offset`.  WRITE true: the write step, after the scan.
template <bool WRITE>
__global__ __launch_bounds__(64 * kMotionWavesPerWg) void motion_pack_kernel(const x266_me_result_t *__restrict__ mv, const uint8_t *__restrict__ level,
                                                                            x266_motion_ctu_t *ctu, uint16_t *__restrict__ stream, int bw, int bh,
                                                                            size_t n_ctu, uint64_t cap_words)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t c = (size_t)blockIdx.x * kMotionWavesPerWg + wave_in_wg;
    if (c >= n_ctu) return;                                                 // wave-uniform; no barrier follows
    uint64_t offset = 0;
    if (WRITE) {
        const uint32_t n_words = ctu[c].n_words;
        offset = ctu[c].offset;
        if (n_words == 0 || offset > cap_words || n_words > cap_words - offset) return;     // wave-uniform: the payload does not fit
    }
    const MotionCtu g = motion_ctu(bw, bh, c);
    const bool exists = motion_block_exists(g, lane);
    const int X = motion_block_x(g, lane), Y = motion_block_y(g, lane);
    const int own = exists ? (int)(level[(size_t)Y * (size_t)bw + (size_t)X] & 3u) : 0;
    int lv[kPartLevels];
    lv[0] = own;
#pragma unroll
    for (int k = 1; k < kPartLevels; ++k) lv[k] = __shfl(own, (int)motion_node_first(lane, k));     // every lane takes part
    const int k = motion_part_level(g, lane, lv);
    const bool head = exists && motion_node_first(lane, k) == lane;
    const uint64_t head_mask = __ballot(head);
    const uint32_t parts = (uint32_t)__popcll(head_mask);
    uint32_t bits = 0, top = 0;
    if (head) {
        const PartVec q = motion_vec_at(mv, bw, X, Y), p = motion_predictor(mv, bw, X, Y, 1 << k);
        const int dx = q.x - p.x, dy = q.y - p.y;                           // the true differences, |d| <= 65535
        if (WRITE) {
            if (4u * parts <= cap_words - offset) {                         // as counted; held against the capacity again all the same
                uint2 w;
                w.x = ((uint32_t)q.x & 0xFFFFu) | (uint32_t)q.y << 16;
                w.y = ((uint32_t)dx & 0xFFFFu) | (uint32_t)dy << 16;
                // 8-byte aligned: d_stream is 16-byte aligned and offset a multiple of four words
                *reinterpret_cast<uint2 *>(stream + offset + (size_t)kMotionWordsPerPart * motion_parts_below(head_mask, lane)) = w;
            }
        } else {
            bits = motion_part_bits(g, lane, k, dx, dy);
            top = motion_abs(dx) > motion_abs(dy) ? motion_abs(dx) : motion_abs(dy);
        }
    }
    if (WRITE) return;
    bits = wave_sum(bits);
    top = wave_max(top);
    if (lane == 0) {
        x266_motion_ctu_t *rec = ctu + c;
        rec->head_mask = head_mask;
        rec->n_words = (uint32_t)kMotionWordsPerPart * parts;
        rec->parts = parts;
        rec->bits = bits;
        rec->max_abs = top;
    }
}

// Trusts head_mask and offset alone.  A CTU whose mask is malformed or whose payload does not lie inside cap_words is written as
// vector (0, 0), cost 0, level 0; words 2 and 3 of a partition are never read, nor anything outside [0, cap_words).
__global__ __launch_bounds__(64 * kMotionWavesPerWg) void motion_unpack_kernel(x266_me_result_t *__restrict__ mv, uint8_t *__restrict__ level,
                                                                              const x266_motion_ctu_t *__restrict__ ctu, const uint16_t *__restrict__ stream,
                                                                              int bw, int bh, size_t n_ctu, uint64_t cap_words)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t c = (size_t)blockIdx.x * kMotionWavesPerWg + wave_in_wg;
    if (c >= n_ctu) return;                                                 // wave-uniform; no barrier follows
    const uint64_t head_mask = ctu[c].head_mask, offset = ctu[c].offset;
    const MotionCtu g = motion_ctu(bw, bh, c);
    const bool exists = motion_block_exists(g, lane);
    const uint64_t exist_mask = __ballot(exists);
    const uint64_t uncovered = __ballot(!motion_block_covered(g, head_mask, lane));
    const uint64_t n_words = (uint64_t)kMotionWordsPerPart * (uint64_t)__popcll(head_mask);          // at most 256: no sum below can wrap
    const bool ok = motion_mask_plausible(head_mask, exist_mask) && uncovered == 0 && offset <= cap_words && n_words <= cap_words - offset;
    if (!exists) return;
    uint2 rec = {0u, 0u};                                                   // mvx | mvy << 16, cost = 0
    uint8_t lvl = 0;
    if (ok) {
        const unsigned h = (unsigned)motion_head_of(head_mask, lane);       // there is one: the mask is well formed
        const uint16_t *at = stream + offset + (size_t)kMotionWordsPerPart * motion_parts_below(head_mask, h);
        rec.x = (uint32_t)at[0] | (uint32_t)at[1] << 16;                    // 16-bit loads: an offset from a host decoder has no alignment
        lvl = (uint8_t)motion_head_level(g, head_mask, h);
    }
    const size_t b = (size_t)motion_block_y(g, lane) * (size_t)bw + (size_t)motion_block_x(g, lane);
    *reinterpret_cast<uint2 *>(mv + b) = rec;
    level[b] = lvl;
}

}  // namespace

hipError_t launch_motion_pack(const x266_motion_t &p, hipStream_t stream)
{
    const int bw = p.width / 8, bh = p.height / 8;
    const size_t n_ctu = (size_t)motion_ctus_w(bw) * (size_t)motion_ctus_h(bh);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(n_ctu, kMotionWavesPerWg, &wgs)) return e;
    const dim3 block(64 * kMotionWavesPerWg);
    hipLaunchKernelGGL(motion_pack_kernel<false>, dim3(wgs), block, 0, stream, (const x266_me_result_t *)p.d_mv, (const uint8_t *)p.d_level, p.d_ctu,
                       (uint16_t *)nullptr, bw, bh, n_ctu, (uint64_t)0);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(levels_scan_kernel<x266_motion_ctu_t>, dim3(1), dim3(kLevelsScanChunk), 0, stream, p.d_ctu, n_ctu, p.cap_words, p.d_total);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.cap_words && p.d_stream)
        hipLaunchKernelGGL(motion_pack_kernel<true>, dim3(wgs), block, 0, stream, (const x266_me_result_t *)p.d_mv, (const uint8_t *)p.d_level, p.d_ctu,
                           p.d_stream, bw, bh, n_ctu, p.cap_words);
    return hipGetLastError();
}

hipError_t launch_motion_unpack(const x266_motion_t &p, hipStream_t stream)
{
    const int bw = p.width / 8, bh = p.height / 8;
    const size_t n_ctu = (size_t)motion_ctus_w(bw) * (size_t)motion_ctus_h(bh);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(n_ctu, kMotionWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(motion_unpack_kernel, dim3(wgs), dim3(64 * kMotionWavesPerWg), 0, stream, p.d_mv, p.d_level, (const x266_motion_ctu_t *)p.d_ctu,
                       (const uint16_t *)p.d_stream, bw, bh, n_ctu, p.cap_words);
    return hipGetLastError();
}

}  // namespace x266
