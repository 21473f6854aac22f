// aq_kernels.hip -- source analysis in front of the coding loop (xAqStatsGpu, xAqDecideGpu): per-tile sums and sums of squares of a
// tiled source frame, their frame totals, and from both a Q8 qp offset per tile and a qp byte per region.  The contract is
// include/x266hip.h's, the arithmetic x266_aq.hpp's.
//
// Statistics: a wave takes 4 tiles, lanes 16k .. 16k + 15 tile k.  Lane j of a row reads luma row j (16 bytes) and chroma row j / 2's
// half j & 1 (8 bytes: four (U, V) pairs) -- 384 of the tile's 512 bytes, m_I is never touched.  Sums are v_sad_u8 against 0, squares
// v_dot4_u32_u8 of a dword with itself, U and V split by their byte masks; the row of 16 lanes is summed by DPP and its first lane
// writes the 32-byte record.  Totals: ONE workgroup walks the records kAqTotalsChunk at a time, as a linear stream of 16-byte halves --
// integer sums in a fixed order, no atomics (workgroup_totals, x266_lanes.hpp).  Decide: 16 lanes per CTU, one per tile (ctu_lane, x266_ctu_tiles.hpp); the quadrant and CTU sums are four xor-shuffles inside the row (aq_ctu_qp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_aq.hpp"
#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"

namespace x266 {
namespace {

typedef unsigned v2u __attribute__((ext_vector_type(2)));
constexpr unsigned kAqWavesPerWg = 4;
static_assert(sizeof(x266_aq_tile_t) == 32, "the record is 32 bytes");
static_assert(sizeof(x266_ref_block_t) == 512, "a tile is 512 bytes");

__global__ __launch_bounds__(64 * kAqWavesPerWg) void aq_stats_kernel(const x266_ref_block_t *__restrict__ src, x266_aq_tile_t *__restrict__ tile,
                                                                      size_t n_tiles)
{
    const unsigned lane = threadIdx.x & 63, row = lane & 15;
    const size_t wave = (size_t)blockIdx.x * kAqWavesPerWg + (threadIdx.x >> 6);
    const size_t t = wave * 4 + (lane >> 4);
    const bool active = t < n_tiles;                                        // uniform over the row of 16 lanes
    v4i y = {0, 0, 0, 0};
    v2u c = {0u, 0u};
    if (active) {                                                           // plain loads: the searches and the coding calls read the frame next
        const uint8_t *base = reinterpret_cast<const uint8_t *>(src + t);
        y = load16<false>(base + row * 16);
        c = *reinterpret_cast<const v2u *>(base + 256 + row * 8);
    }
    uint32_t sum_y = 0, ssq_y = 0, sum_uv = 0, ssq_u = 0, ssq_v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = (uint32_t)y[i];
        sum_y = __builtin_amdgcn_sad_u8(w, 0u, sum_y);
        ssq_y = __builtin_amdgcn_udot4(w, w, ssq_y, false);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t w = i ? c.y : c.x, u = w & 0x00FF00FFu, v = w & 0xFF00FF00u;
        sum_uv = __builtin_amdgcn_sad_u8(u, 0u, sum_uv);                    // a row's U sum is at most 64 * 255 < 2^16: U and V share a register
        sum_uv += __builtin_amdgcn_sad_u8(v, 0u, 0u) << 16;
        ssq_u = __builtin_amdgcn_udot4(u, u, ssq_u, false);
        ssq_v = __builtin_amdgcn_udot4(v, v, ssq_v, false);
    }
    sum_y = sum_over_row16(sum_y);
    ssq_y = sum_over_row16(ssq_y);
    sum_uv = sum_over_row16(sum_uv);
    ssq_u = sum_over_row16(ssq_u);
    ssq_v = sum_over_row16(ssq_v);
    if (active && row == 0) {
        const uint32_t sum_u = sum_uv & 0xFFFFu, sum_v = sum_uv >> 16;
        const uint32_t energy = aq_energy(sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v);
        v4i *rec = reinterpret_cast<v4i *>(tile + t);
        const v4i lo = {(int)sum_y, (int)ssq_y, (int)sum_u, (int)ssq_u}, hi = {(int)sum_v, (int)ssq_v, (int)energy, (int)aq_log2_q8(energy)};
        rec[0] = lo;
        rec[1] = hi;
    }
}

// total[0..5] = the six sums over all records, total[6] = the sum of log2_q8, total[7] = n_tiles.  One workgroup.
// The records are read as one stream of 16-byte halves, lane after lane: an even lane only ever sees first halves (sum_y, ssq_y, sum_u,
// ssq_u), an odd lane second halves (sum_v, ssq_v, energy, log2_q8), because every stride is even.  A full step is four loads per lane in
// flight: kAqTotalsChunk records.
__global__ __launch_bounds__(kAqTotalsThreads) void aq_totals_kernel(const x266_aq_tile_t *__restrict__ tile, size_t n_tiles, int64_t *__restrict__ total)
{
    constexpr unsigned kWaves = kAqTotalsThreads / 64;
    static_assert(kAqTotalsThreads % 2 == 0 && 4 * kAqTotalsThreads == 2 * kAqTotalsChunk, "a full step is four halves per lane, of one parity");
    const unsigned tid = threadIdx.x;
    const v4i *half = reinterpret_cast<const v4i *>(tile);
    const size_t n_halves = n_tiles * 2;
    uint64_t acc[4] = {0, 0, 0, 0};
    auto add = [&acc](const v4i &v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += (uint32_t)v[k];
    };
    size_t j = tid;
    for (; j + 3 * kAqTotalsThreads < n_halves; j += 4 * kAqTotalsThreads) {
        const v4i a = half[j], b = half[j + kAqTotalsThreads], c = half[j + 2 * kAqTotalsThreads], d = half[j + 3 * kAqTotalsThreads];
        add(a);
        add(b);
        add(c);
        add(d);
    }
    for (; j < n_halves; j += kAqTotalsThreads) add(half[j]);
    const uint64_t all = workgroup_totals<kWaves, 2>(acc, tid);               // slots 0..3 the even lanes' sums, 4..7 the odd lanes': a record's words
    if (tid < 8) {
        if (tid < 6) total[tid] = (int64_t)all;                             // the six sums
        if (tid == 7) total[6] = (int64_t)all;                              // log2_q8; word 6 of a record, the energy, has no total
        if (tid == 6) total[7] = (int64_t)n_tiles;
    }
}

// a row of 16 lanes per CTU, lane i its tile (i & 3, i >> 2)
__global__ __launch_bounds__(64 * kAqWavesPerWg) void aq_decide_kernel(const x266_aq_tile_t *__restrict__ tile, const int64_t *__restrict__ total, TileFrame f,
                                                                       int mode, int strength_q8, int base_qp, int chroma_qp_offset,
                                                                       int16_t *__restrict__ offset, uint8_t *__restrict__ qp)
{
    const CtuLane m = ctu_lane(threadIdx.x, blockIdx.x, kAqWavesPerWg, f);
    const size_t n_tiles = (size_t)f.tiles_w * f.tiles_h;
    const int ref_q8 = aq_ref_q8(mode, mode == 1 ? 0 : total[6], (int64_t)n_tiles);
    int s = 0, n = 0;
    if (m.in_frame) {
        s = aq_offset_q8(strength_q8, (int)tile[m.t].log2_q8, ref_q8);
        n = 1;
        if (offset) offset[m.t] = (int16_t)s;
    }
    aq_ctu_qp(s, n, threadIdx.x & 63, m.ctu_ok, m.ctu, base_qp, chroma_qp_offset, qp);
}

}  // namespace

int aq_totals_chunk() { return (int)kAqTotalsChunk; }

hipError_t launch_aq_stats(const x266_aq_t &p, hipStream_t stream)
{
    const size_t n_tiles = (size_t)(p.width / 16) * (size_t)(p.height / 16);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((n_tiles + 3) / 4, kAqWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(aq_stats_kernel, dim3(wgs), dim3(64 * kAqWavesPerWg), 0, stream, p.d_src, p.d_tile, n_tiles);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(aq_totals_kernel, dim3(1), dim3(kAqTotalsThreads), 0, stream, p.d_tile, n_tiles, p.d_total);
    return hipGetLastError();
}

hipError_t launch_aq_decide(const x266_aq_t &p, hipStream_t stream)
{
    const TileFrame f = tile_frame(p.width, p.height);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((f.n_ctu + 3) / 4, kAqWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(aq_decide_kernel, dim3(wgs), dim3(64 * kAqWavesPerWg), 0, stream, p.d_tile, p.d_total, f, p.mode, p.strength_q8, p.qp, p.chroma_qp_offset,
                       p.d_offset, p.d_qp);
    return hipGetLastError();
}

}  // namespace x266
