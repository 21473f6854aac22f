// lookahead_kernels.hip -- the lookahead (xLaDownscaleGpu, xLaIntraCostsGpu, xLaFrameCostGpu, xLaPropagateGpu, xLaTreeQpGpu): a half-size
// copy of a tiled frame, the open-loop intra cost of its 8x8 blocks, the per-block choice between intra and the two lists with its frame
// totals, one step of the propagation tree, and the qp map from what the tree accumulated.  The contract is include/x266hip.h's, the
// arithmetic x266_lookahead.hpp's.
//
// Downscale: a wave takes 4 output tiles, lanes 16k .. 16k + 15 tile k, as aq_kernels.hip maps a tile.  Lane r writes luma row r (from
// two rows of the two input tiles side by side: four 16-byte loads) and half r & 1 of chroma row r >> 1 (two rows of one input tile:
// two 16-byte loads) -- 4 x 384 bytes read per output tile, m_I never touched.
// Intra costs: a wave takes 8 blocks, 8 lanes each, lane y row y.  A lane forms its row of each candidate, transforms the difference
// along the row, and the columns run across the 8 lanes: three xor-shuffles of four registers holding two 16-bit coefficients each.
// Frame cost: a lane per block; totals: ONE workgroup walks the records kLaTotalsChunk at a time -- integer sums in a fixed order, no
// atomics (workgroup_totals, x266_lanes.hpp).  Propagate: a lane per block, up to four 64-bit atomic adds (no return value).  Tree qp: 16
// lanes per CTU, one per tile (ctu_lane, x266_ctu_tiles.hpp), and the source analysis' reduction (aq_ctu_qp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"
#include "x266_lookahead.hpp"

namespace x266 {
namespace {

typedef short v2s __attribute__((ext_vector_type(2)));
constexpr unsigned kLaWavesPerWg = 4;
static_assert(sizeof(x266_la_block_t) == 16, "the record is 16 bytes");
static_assert(sizeof(x266_me_result_t) == 8, "a search record is 8 bytes");
static_assert(sizeof(x266_ref_block_t) == 512, "a tile is 512 bytes");

// ---- 1. downscale --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kLaWavesPerWg) void la_downscale_kernel(const x266_ref_block_t *__restrict__ src, x266_ref_block_t *__restrict__ low,
                                                                          unsigned low_tiles_w, size_t n_low)
{
    const unsigned lane = threadIdx.x & 63, r = lane & 15;
    const size_t wave = (size_t)blockIdx.x * kLaWavesPerWg + (threadIdx.x >> 6);
    const size_t t = wave * 4 + (lane >> 4);
    if (t >= n_low) return;
    const size_t ty = t / low_tiles_w, tx = t % low_tiles_w;
    const size_t src_tiles_w = (size_t)low_tiles_w * 2;
    // luma row r of the output: input rows 2r and 2r + 1, that is rows (2r & 15) and + 1 of the input tiles (2 tx, 2 ty + (r >> 3)) and the one right of it
    const uint8_t *left = reinterpret_cast<const uint8_t *>(src + (2 * ty + (r >> 3)) * src_tiles_w + 2 * tx);
    const unsigned row = (2 * r) & 15;
    const v4i a0 = load16<false>(left + row * 16), a1 = load16<false>(left + row * 16 + 16);
    const v4i b0 = load16<false>(left + 512 + row * 16), b1 = load16<false>(left + 512 + row * 16 + 16);
    // chroma row c = r >> 1, half k = r & 1 (4 of its 8 pairs): input chroma rows 2c and 2c + 1, all 8 pairs, of the input tile (2 tx + k, 2 ty + (c >> 2))
    const unsigned c = r >> 1, k = r & 1, crow = (2 * c) & 7;
    const uint8_t *ctile = reinterpret_cast<const uint8_t *>(src + (2 * ty + (c >> 2)) * src_tiles_w + 2 * tx + k) + 256;
    const v4i c0 = load16<false>(ctile + crow * 16), c1 = load16<false>(ctile + crow * 16 + 16);
    v4i y;
    y[0] = (int)la_box_luma((uint32_t)a0[0], (uint32_t)a0[1], (uint32_t)a1[0], (uint32_t)a1[1]);
    y[1] = (int)la_box_luma((uint32_t)a0[2], (uint32_t)a0[3], (uint32_t)a1[2], (uint32_t)a1[3]);
    y[2] = (int)la_box_luma((uint32_t)b0[0], (uint32_t)b0[1], (uint32_t)b1[0], (uint32_t)b1[1]);
    y[3] = (int)la_box_luma((uint32_t)b0[2], (uint32_t)b0[3], (uint32_t)b1[2], (uint32_t)b1[3]);
    uint2 uv;
    uv.x = la_box_chroma((uint32_t)c0[0], (uint32_t)c0[1], (uint32_t)c1[0], (uint32_t)c1[1]);
    uv.y = la_box_chroma((uint32_t)c0[2], (uint32_t)c0[3], (uint32_t)c1[2], (uint32_t)c1[3]);
    uint8_t *out = reinterpret_cast<uint8_t *>(low + t);
    store16<false>(out + r * 16, y);                                        // plain stores: the intra costs and the search read the frame next
    *reinterpret_cast<uint2 *>(out + 256 + c * 16 + k * 8) = uv;
}

// ---- 2. intra costs ------------------------------------------------------------------------------------------------------------------------
// sum |H| of the block whose row-transformed differences the 8 lanes of a group hold (lane y row y); every lane of the group gets it
__device__ __forceinline__ uint32_t la_sum_abs_columns(const int h[8], unsigned y)
{
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v2s v = {(short)h[2 * k], (short)h[2 * k + 1]};                     // |h| <= 8 * 255, and 64 * 255 after the columns: 16 bits hold both
#pragma unroll
        for (unsigned d = 1; d < 8; d <<= 1) {
            const v2s o = __builtin_bit_cast(v2s, __shfl_xor(__builtin_bit_cast(int, v), (int)d, 64));
            v = (y & d) ? o - v : v + o;
        }
        sum += (uint32_t)(v.x < 0 ? -v.x : v.x) + (uint32_t)(v.y < 0 ? -v.y : v.y);
    }
    sum += (uint32_t)__shfl_xor((int)sum, 1, 64);
    sum += (uint32_t)__shfl_xor((int)sum, 2, 64);
    sum += (uint32_t)__shfl_xor((int)sum, 4, 64);
    return sum;
}

__global__ __launch_bounds__(64 * kLaWavesPerWg) void la_intra_costs_kernel(const x266_ref_block_t *__restrict__ low, unsigned low_w, unsigned low_h,
                                                                            size_t n_blocks, uint32_t *__restrict__ intra, uint8_t *__restrict__ mode)
{
    const unsigned lane = threadIdx.x & 63, y = lane & 7;
    const size_t wave = (size_t)blockIdx.x * kLaWavesPerWg + (threadIdx.x >> 6);
    const size_t b = wave * 8 + (lane >> 3);
    const bool active = b < n_blocks;                                       // uniform over the group of 8 lanes; an idle group shuffles zeros
    const unsigned blocks_w = low_w >> 3;
    const unsigned x0 = active ? (unsigned)(b % blocks_w) * 8 : 0, y0 = active ? (unsigned)(b / blocks_w) * 8 : 0;
    const uint8_t *luma = reinterpret_cast<const uint8_t *>(low);
    int cur[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    LaEdge e = {};
    if (active) {
        const uint2 w = *reinterpret_cast<const uint2 *>(luma + la_luma_at(x0, y0 + y, low_w >> 4));   // 8 samples of a tile row, 8-byte aligned
#pragma unroll
        for (int x = 0; x < 8; ++x) cur[x] = (int)(((x < 4 ? w.x : w.y) >> (8 * (x & 3))) & 255u);
        e = la_edge(luma, x0, y0, y, low_w, low_h);
    }
    uint32_t best = 0;
    unsigned best_mode = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int d[8];
        la_pred_row(c, (int)y, e, d);
#pragma unroll
        for (int x = 0; x < 8; ++x) d[x] = cur[x] - d[x];
        la_hadamard8(d);
        const uint32_t cost = la_satd_round(la_sum_abs_columns(d, y));
        if (c == 0 || cost < best) {                                        // the first of equal costs stays
            best = cost;
            best_mode = la_mode_number(c);
        }
    }
    if (active && y == 0) {
        intra[b] = best;
        if (mode) mode[b] = (uint8_t)best_mode;
    }
}

// ---- 3. frame cost -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void la_frame_cost_kernel(const uint32_t *__restrict__ intra, const uint8_t *__restrict__ mode,
                                                            const x266_me_result_t *__restrict__ inter0, const x266_me_result_t *__restrict__ inter1,
                                                            uint32_t intra_penalty, size_t n_blocks, x266_la_block_t *__restrict__ block)
{
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    x266_me_result_t l0 = {}, l1 = {};
    if (inter0) l0 = inter0[b];
    if (inter1) l1 = inter1[b];
    const x266_la_block_t r = la_decide(intra[b], mode ? mode[b] : 0u, inter0 != nullptr, l0, inter1 != nullptr, l1, intra_penalty);
    v4i out;
    out[0] = (int)r.cost;
    out[1] = (int)r.intra;
    out[2] = (int)((uint32_t)(uint16_t)r.mvx | ((uint32_t)(uint16_t)r.mvy << 16));
    out[3] = (int)((uint32_t)r.kind | ((uint32_t)r.mode << 8));             // reserved = 0
    *reinterpret_cast<v4i *>(block + b) = out;
}

// total[0] = sum of cost, [1] of intra, [2..4] the numbers of kind 0 / 1 / 2, [5] / [6] the lists' costs over all blocks, [7] = n_blocks.
// One workgroup; a full step is two blocks per lane, kLaTotalsChunk in all.
__global__ __launch_bounds__(kLaTotalsThreads) void la_totals_kernel(const x266_la_block_t *__restrict__ block, const x266_me_result_t *__restrict__ inter0,
                                                                     const x266_me_result_t *__restrict__ inter1, size_t n_blocks, int64_t *__restrict__ total)
{
    constexpr unsigned kWaves = kLaTotalsThreads / 64;
    static_assert(2 * kLaTotalsThreads == kLaTotalsChunk, "a full step is two blocks per lane");
    const unsigned tid = threadIdx.x;
    uint64_t acc[7] = {0, 0, 0, 0, 0, 0, 0};
    auto add = [&](size_t j) {
        const v4i r = *reinterpret_cast<const v4i *>(block + j);
        const unsigned kind = (uint32_t)r[3] & 255u;
        acc[0] += (uint32_t)r[0];
        acc[1] += (uint32_t)r[1];
        acc[2] += kind == 0;
        acc[3] += kind == 1;
        acc[4] += kind == 2;
        if (inter0) acc[5] += inter0[j].cost;
        if (inter1) acc[6] += inter1[j].cost;
    };
    size_t j = tid;
    for (; j + kLaTotalsThreads < n_blocks; j += 2 * kLaTotalsThreads) {
        add(j);
        add(j + kLaTotalsThreads);
    }
    for (; j < n_blocks; j += kLaTotalsThreads) add(j);
    const uint64_t all = workgroup_totals<kWaves>(acc, tid);
    if (tid < 8) total[tid] = (int64_t)(tid < 7 ? all : n_blocks);
}

// ---- 5. one step of the propagation tree -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void la_propagate_kernel(const x266_la_block_t *__restrict__ block, const uint64_t *__restrict__ prop, int blocks_w,
                                                           int blocks_h, unsigned long long *ref0, unsigned long long *ref1)
{
    const size_t n_blocks = (size_t)blocks_w * (size_t)blocks_h;
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const v4i r = *reinterpret_cast<const v4i *>(block + b);
    const uint32_t cost = (uint32_t)r[0], intra = (uint32_t)r[1];
    const unsigned kind = (uint32_t)r[3] & 255u;
    unsigned long long *ref = kind == 1 ? ref0 : kind == 2 ? ref1 : nullptr;
    if (!ref || intra == 0) return;
    const int mvx = (int16_t)((uint32_t)r[2] & 0xFFFFu), mvy = (int16_t)((uint32_t)r[2] >> 16);
    const uint64_t amount = la_amount(cost, intra, prop ? prop[b] : 0);
    const LaTargets t = la_targets((int)(b % (size_t)blocks_w), (int)(b / (size_t)blocks_w), mvx, mvy, blocks_w, blocks_h, amount);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.index[k] >= 0) atomicAdd(ref + t.index[k], (unsigned long long)t.share[k]);      // the result is not used: no return value
}

// ---- 6. the qp map -------------------------------------------------------------------------------------------------------------------------
// a row of 16 lanes per CTU, lane i its tile (i & 3, i >> 2), as the source analysis' decision
__global__ __launch_bounds__(64 * kLaWavesPerWg) void la_tree_qp_kernel(const x266_la_block_t *__restrict__ block, const uint64_t *__restrict__ prop,
                                                                        const int16_t *__restrict__ aq_offset, TileFrame f, int strength_q8, int base_qp,
                                                                        int chroma_qp_offset, int16_t *__restrict__ offset, uint8_t *__restrict__ qp)
{
    const CtuLane m = ctu_lane(threadIdx.x, blockIdx.x, kLaWavesPerWg, f);
    const size_t t = m.t;
    int s = 0, n = 0;
    if (m.in_frame) {
        s = la_tree_offset_q8(aq_offset ? (int)aq_offset[t] : 0, la_gain_q8(block[t].intra, prop ? prop[t] : 0, strength_q8));
        n = 1;
        if (offset) offset[t] = (int16_t)s;
    }
    aq_ctu_qp(s, n, threadIdx.x & 63, m.ctu_ok, m.ctu, base_qp, chroma_qp_offset, qp);
}

}  // namespace

int la_totals_chunk() { return (int)kLaTotalsChunk; }

static size_t la_blocks(const x266_la_t &p) { return (size_t)(p.width / 16) * (size_t)(p.height / 16); }

hipError_t launch_la_downscale(const x266_la_t &p, hipStream_t stream)
{
    const size_t n_low = la_blocks(p) / 4;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((n_low + 3) / 4, kLaWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(la_downscale_kernel, dim3(wgs), dim3(64 * kLaWavesPerWg), 0, stream, p.d_src, p.d_low, (unsigned)(p.width / 32), n_low);
    return hipGetLastError();
}

hipError_t launch_la_intra_costs(const x266_la_t &p, hipStream_t stream)
{
    const size_t n = la_blocks(p);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((n + 7) / 8, kLaWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(la_intra_costs_kernel, dim3(wgs), dim3(64 * kLaWavesPerWg), 0, stream, p.d_low, (unsigned)(p.width / 2), (unsigned)(p.height / 2), n,
                       p.d_intra, p.d_mode);
    return hipGetLastError();
}

hipError_t launch_la_frame_cost(const x266_la_t &p, hipStream_t stream)
{
    const size_t n = la_blocks(p);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((n + 63) / 64, 4, &wgs)) return e;
    hipLaunchKernelGGL(la_frame_cost_kernel, dim3(wgs), dim3(256), 0, stream, p.d_intra, p.d_mode, p.d_inter0, p.d_inter1, (uint32_t)p.intra_penalty, n, p.d_block);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(la_totals_kernel, dim3(1), dim3(kLaTotalsThreads), 0, stream, p.d_block, p.d_inter0, p.d_inter1, n, p.d_total);
    return hipGetLastError();
}

hipError_t launch_la_propagate(const x266_la_t &p, hipStream_t stream)
{
    if (!p.d_prop_ref0 && !p.d_prop_ref1) return hipSuccess;               // nothing to add into
    const size_t n = la_blocks(p);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((n + 63) / 64, 4, &wgs)) return e;
    hipLaunchKernelGGL(la_propagate_kernel, dim3(wgs), dim3(256), 0, stream, p.d_block, p.d_prop, p.width / 16, p.height / 16,
                       reinterpret_cast<unsigned long long *>(p.d_prop_ref0), reinterpret_cast<unsigned long long *>(p.d_prop_ref1));
    return hipGetLastError();
}

hipError_t launch_la_tree_qp(const x266_la_t &p, hipStream_t stream)
{
    const TileFrame f = tile_frame(p.width, p.height);
    unsigned wgs = 0;
    if (hipError_t e = wave_grid((f.n_ctu + 3) / 4, kLaWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(la_tree_qp_kernel, dim3(wgs), dim3(64 * kLaWavesPerWg), 0, stream, p.d_block, p.d_prop, p.d_aq_offset, f, p.strength_q8, p.qp,
                       p.chroma_qp_offset, p.d_offset, p.d_qp);
    return hipGetLastError();
}

}  // namespace x266
