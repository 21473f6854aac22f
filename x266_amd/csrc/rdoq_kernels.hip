// rdoq_kernels.hip -- rate-distortion optimised quantisation of 1024-coefficient regions (xRdoQuantRegionsGpu), the rate estimate of
// a region's levels (xLevelsBitsGpu) and the choice of each region's transform class by rate-distortion cost
// (xTransformDecideCtuTilesGpu).  The contract is include/x266hip.h's, the arithmetic x266_rdoq.hpp's, the scan x266_levels.hpp's; the
// per-wave pieces are x266_rdoq_blocks.hpp's and, for the decision's transforms, x266_transform_blocks.hpp's.
//
// One region per wave, four waves per workgroup, lane g = CG bit g (the compact level stream's arrangement): a block of N = 4 << k is
// a segment of (N / 4)^2 = 1, 4, 16 or 64 consecutive lanes whose order is the block's CG scan.  The memory side is the plain
// quantiser's -- two 1 KiB-linear 16-byte loads and stores per lane -- and the region crosses an LDS slab of the wave's own to reach
// the CG-per-lane arrangement (four 8-byte LDS accesses per lane each way).  In place is safe: a wave has read its whole region
// before it writes any of it.
//   step 1  lane-local: 16 coefficients, two or three candidates each; the lane keeps q, D(q) | R(q) << 20 and D(0) per position
//   step 2  one 64-bit comparison per lane
//   step 3  an inclusive scan of (C(s), sum D(0)) over the segment's lanes (__shfl_up, 64-bit pairs), each lane's at most 16
//           candidate totals in scan order with "<=" (the later position wins a tie), then the minimum of (Total, lane) across the
//           segment by butterfly (__shfl_xor; the higher lane wins a tie).  Every lane of the segment ends with the same winner.
// No atomics, no ordering between waves: the bytes depend on the data alone.  The class and qp bytes are scalar loads (uniform_byte),
// and QuantParams are computed on the scalar side.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_levels.hpp"
#include "x266_quant.hpp"
#include "x266_rdoq.hpp"
#include "x266_rdoq_blocks.hpp"
#include "x266_transform_blocks.hpp"

namespace x266 {
namespace {

__global__ __launch_bounds__(64 * kRdoqWavesPerWg) void rdoq_regions_kernel(const int16_t *coef, int16_t *level, size_t n_regions,
                                                                           const uint8_t *__restrict__ cls, const uint8_t *__restrict__ qps, unsigned qp,
                                                                           unsigned lambda, uint32_t *__restrict__ nnz, x266_rdoq_region_t *__restrict__ stat)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kRdoqWavesPerWg][kRdoqRegionBytes];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kRdoqWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;                                      // wave-uniform; every wave reaches both barriers
    char *slab = lds_region[wave_in_wg];
    if (active) rdoq_region_to_lds(coef, r, lane, slab);
    __syncthreads();
    unsigned k = 3u, q = 0u;
    if (active) {
        const unsigned cls_byte = cls ? uniform_byte(cls, r) : 3u, qp_byte = qps ? uniform_byte(qps, r) : qp;
        k = cls_byte & 3u;
        q = qp_byte < 51u ? qp_byte : 51u;
    }
    const QuantParams qpar = quant_params(k + 2u, q, kRdoqRoundNearest);
    const unsigned origin = level_cg_origin(k, lane);
    int l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) l[i] = 0;
    if (active) rdoq_cg_from_lds(slab, origin, 4u << k, l);
    const CgPlace place = cg_place(k, lane, origin);
    const RdoqLane mine = rdoq_steps(l, k, lane, place, qpar, lambda);      // here, so that the per-position arrays die before the barrier
    if (active) rdoq_cg_to_lds(slab, origin, 4u << k, l);
    __syncthreads();
    if (!active) return;
    char *dst = reinterpret_cast<char *>(level) + r * kRdoqRegionBytes + lane * 16;
    store16_sc1nt(dst, *reinterpret_cast<const v4i *>(slab + lane * 16));
    store16_sc1nt(dst + 1024, *reinterpret_cast<const v4i *>(slab + 1024 + lane * 16));
    const uint32_t n_nz = wave_sum(mine.count);
    if (nnz && lane == 0) nnz[r] = n_nz;
    if (stat) {
        const uint32_t bits = wave_sum(mine.bits);
        const uint64_t total = wave_sum(mine.dist);
        if (lane == 0) {
            stat[r].dist = total;
            stat[r].bits = bits;
            stat[r].n_nz = n_nz;
        }
    }
}

__global__ __launch_bounds__(64 * kRdoqWavesPerWg) void levels_bits_kernel(const int16_t *__restrict__ level, size_t n_regions, const uint8_t *__restrict__ cls,
                                                                          const uint32_t *__restrict__ nnz, x266_rdoq_region_t *__restrict__ stat)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kRdoqWavesPerWg][kRdoqRegionBytes];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kRdoqWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;
    bool skip = !active;                                                    // wave-uniform: no level of the region is read
    if (active && nnz && nnz[r] == 0) skip = true;
    char *slab = lds_region[wave_in_wg];
    if (!skip) rdoq_region_to_lds(level, r, lane, slab);
    __syncthreads();
    const unsigned k = (active && cls) ? (uniform_byte(cls, r) & 3u) : 3u;
    const unsigned origin = level_cg_origin(k, lane);
    int l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) l[i] = 0;
    if (!skip) rdoq_cg_from_lds(slab, origin, 4u << k, l);
    const CgPlace place = cg_place(k, lane, origin);
    unsigned rate[16], map = 0;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const int v = l[level_scan4(i)];
        rate[i] = rdoq_level_bits((unsigned)(v < 0 ? -v : v), i ? place.sig0 : place.sig0_dc, i ? place.sig1 : place.sig1_dc);
        map |= (unsigned)(v != 0) << i;
    }
    const int last = segment_last_lane(map != 0, lane, 1u << (2u * k));
    const unsigned p = map ? 31u - (unsigned)__builtin_clz(map) : 0u;
    const uint32_t bits = wave_sum(last >= 0 ? cg_bits(rate, map, place, lane, last, p) : 0u);
    const uint32_t n_nz = wave_sum((uint32_t)__popc(map));
    if (active && lane == 0) {
        stat[r].dist = 0;
        stat[r].bits = bits;
        stat[r].n_nz = n_nz;
    }
}

// ---- the transform decision (xTransformDecideCtuTilesGpu) ------------------------------------------------------------------------------
// One region per wave.  The lane's 16 residuals of its row segment (lane (c, h): row c, columns 16h .. 16h+15, as in
// tr_ctu_from_tiles_kernel) stay in registers; per candidate class, in ascending order, they go into the wave's one 2 KiB slot in that
// class's block-major layout, the forward tile pipeline turns the slot into coefficients in place, and the same slot is then the RDOQ
// slab: the lane reads its CG and runs rdoq_steps.  J is wave-uniform, so is the comparison; the best levels so far are kept packed,
// 8 dwords per lane, in the CG arrangement of their class, and only the winner reaches memory.  LDS per wave: table 2 KiB + slot 2 KiB.
struct TDecideArgs {
    const x266_ref_block_t *cur, *pred;
    const uint8_t *qps;
    const uint8_t *cand;               // d_cand as bytes: two uniform_byte reads per region, little-endian
    uint8_t *cls;
    int16_t *level;
    uint32_t *nnz;
    x266_rdoq_region_t *stat;
    uint64_t *cost;
    size_t n_regions;
    int ctus_x, tiles_x, tiles_y;
    unsigned qp, lambda, cand_luma, cand_chroma;
    uint32_t class_bits[8];            // two per dword
};

constexpr unsigned kTDecideLdsPerWave = 4096;

__global__ __launch_bounds__(64 * kRdoqWavesPerWg) void tdecide_kernel(const TDecideArgs a, const TileTab *__restrict__ T)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[kRdoqWavesPerWg * kTDecideLdsPerWave];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kRdoqWavesPerWg + wave_in_wg;
    if (r >= a.n_regions) return;                                           // wave-uniform, and the kernel has no workgroup barrier
    unsigned char *tab = stage + wave_in_wg * kTDecideLdsPerWave, *slot = tab + 2048;
    const size_t ctu = r / 6;
    const unsigned q = (unsigned)(r - ctu * 6);
    const unsigned c = lane & 31, h = lane >> 5;
    const CtuPlace at = {ctu / (size_t)a.ctus_x, ctu % (size_t)a.ctus_x, a.tiles_x, a.tiles_y};
    copy_table(tab, T, (int)lane);
    // the lane's residuals: none outside the frame
    uint32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = 0;
    bool inside = true;                                                     // wave-uniform; chroma is never wholly outside
    if (q < 4) {
        inside = at.luma_in(q);
        if (ctu_luma_tile_row(at.cy, q, c) < (size_t)a.tiles_y && ctu_luma_tile_col(at.cx, q, h) < (size_t)a.tiles_x) {
            const size_t off = ctu_luma_tile(at.cy, at.cx, q, c, h, a.tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
            const v4i x = load16<true>(reinterpret_cast<const unsigned char *>(a.cur) + off);
            const v4i z = load16<true>(reinterpret_cast<const unsigned char *>(a.pred) + off);
            luma_residual16(x, z, d);
        }
    } else {
        const bool crow = ctu_chroma_tile_row(at.cy, c) < (size_t)a.tiles_y;
        const size_t coff = ctu_chroma_tile(at.cy, at.cx, c, h, a.tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
        uint32_t du[8], dv[8];
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            v4i x = {0, 0, 0, 0}, z = {0, 0, 0, 0};
            if (crow && ctu_chroma_tile_col(at.cx, h) + j < (size_t)a.tiles_x) {
                x = load16<true>(reinterpret_cast<const unsigned char *>(a.cur) + coff + j * sizeof(x266_ref_block_t));
                z = load16<true>(reinterpret_cast<const unsigned char *>(a.pred) + coff + j * sizeof(x266_ref_block_t));
            }
            chroma_residual8(x, z, du + 4 * j, dv + 4 * j);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = q == 4 ? du[i] : dv[i];
    }
    const unsigned qp_byte = a.qps ? uniform_byte(a.qps, r) : a.qp, qp = qp_byte < 51u ? qp_byte : 51u;
    unsigned mask = a.cand ? (uniform_byte(a.cand, 2 * r) | uniform_byte(a.cand, 2 * r + 1) << 8) & (unsigned)X266_TDECIDE_CLASSES : 0u;
    if (mask == 0) mask = q < 4 ? a.cand_luma : a.cand_chroma;

    uint32_t best[8];                                                       // the best levels so far, l[2 i] | l[2 i + 1] << 16
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = 0;
    uint64_t best_j = UINT64_MAX, best_dist = 0, my_cost = UINT64_MAX;      // my_cost: J of class `lane`
    unsigned best_k = 0, best_bits = 0, best_nz = 0;
    bool have = false;
    for (unsigned k = 0; k < 15; ++k) {                                     // scalar-uniform
        if (!((mask >> k) & 1u)) continue;
        const unsigned kk = k & 3u, origin = level_cg_origin(kk, lane);
        int l[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) l[i] = 0;
        if (inside) {
            __builtin_amdgcn_wave_barrier();                                // the previous candidate has left the slot
            put_segment(slot, (int)k, c, h, d);
            __builtin_amdgcn_wave_barrier();
            fwd_tile_of_any_class(slot, tab, (int)lane, (int)k);
            __builtin_amdgcn_wave_barrier();
            rdoq_cg_from_lds(reinterpret_cast<const char *>(slot), origin, 4u << kk, l);
        }
        const CgPlace place = cg_place(kk, lane, origin);
        const RdoqLane mine = rdoq_steps(l, kk, lane, place, quant_params(kk + 2u, qp, kRdoqRoundNearest), a.lambda);
        const uint32_t bits = wave_sum(mine.bits), n_nz = wave_sum(mine.count);
        uint64_t dist = wave_sum(mine.dist);
        dist = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dist) |
               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(dist >> 32)) << 32;
        const unsigned side = (a.class_bits[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
        const uint64_t j = dist + (uint64_t)a.lambda * (uint64_t)(bits + side);
        if (lane == k) my_cost = j;
        if (!have || j < best_j) {                                          // ascending k: the smallest class byte keeps a tie
            have = true;
            best_j = j;
            best_k = k;
            best_dist = dist;
            best_bits = bits;
            best_nz = n_nz;
#pragma unroll
            for (int i = 0; i < 8; ++i) best[i] = ((uint32_t)l[2 * i] & 0xFFFFu) | ((uint32_t)l[2 * i + 1] << 16);
        }
    }
    // the winner's levels through the slot into its region, 1 KiB-linear
    {
        const unsigned kk = best_k & 3u;
        int l[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            l[2 * i] = (int)(int16_t)(best[i] & 0xFFFFu);
            l[2 * i + 1] = (int)best[i] >> 16;
        }
        __builtin_amdgcn_wave_barrier();
        rdoq_cg_to_lds(reinterpret_cast<char *>(slot), level_cg_origin(kk, lane), 4u << kk, l);
        __builtin_amdgcn_wave_barrier();
        char *dst = reinterpret_cast<char *>(a.level) + r * kRdoqRegionBytes + lane * 16;
        store16_sc1nt(dst, *reinterpret_cast<const v4i *>(slot + lane * 16));
        store16_sc1nt(dst + 1024, *reinterpret_cast<const v4i *>(slot + 1024 + lane * 16));
    }
    if (a.cost && lane < 16) a.cost[r * 16 + lane] = my_cost;
    if (lane == 0) {
        a.cls[r] = (uint8_t)best_k;
        if (a.nnz) a.nnz[r] = best_nz;
        if (a.stat) {
            a.stat[r].dist = best_dist;
            a.stat[r].bits = best_bits;
            a.stat[r].n_nz = best_nz;
        }
    }
}

}  // namespace

hipError_t launch_transform_decide(const x266_tdecide_t &p, const TileTab *d_tab, hipStream_t stream)
{
    TDecideArgs a;
    a.cur = p.d_cur;
    a.pred = p.d_pred;
    a.qps = p.d_qp;
    a.cand = reinterpret_cast<const uint8_t *>(p.d_cand);
    a.cls = p.d_class;
    a.level = p.d_level;
    a.nnz = p.d_nnz;
    a.stat = p.d_stat;
    a.cost = p.d_cost;
    a.ctus_x = (p.width + 63) / 64;
    a.n_regions = 6 * (size_t)a.ctus_x * (size_t)((p.height + 63) / 64);
    a.tiles_x = p.width / 16;
    a.tiles_y = p.height / 16;
    a.qp = (unsigned)p.qp;
    a.lambda = (unsigned)p.lambda;
    a.cand_luma = p.cand_luma;
    a.cand_chroma = p.cand_chroma;
    for (int i = 0; i < 8; ++i) a.class_bits[i] = (uint32_t)p.class_bits[2 * i] | (uint32_t)p.class_bits[2 * i + 1] << 16;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(a.n_regions, kRdoqWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(tdecide_kernel, dim3(wgs), dim3(64 * kRdoqWavesPerWg), 0, stream, a, d_tab);
    return hipGetLastError();
}

hipError_t launch_rdo_quant_regions(const x266_rdoq_t &p, hipStream_t stream)
{
    if (p.n_regions == 0) return hipSuccess;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kRdoqWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(rdoq_regions_kernel, dim3(wgs), dim3(64 * kRdoqWavesPerWg), 0, stream, p.d_coef, p.d_level, p.n_regions, p.d_class, p.d_qp, (unsigned)p.qp,
                       (unsigned)p.lambda, p.d_nnz, p.d_stat);
    return hipGetLastError();
}

hipError_t launch_levels_bits(const x266_rdoq_t &p, hipStream_t stream)
{
    if (p.n_regions == 0) return hipSuccess;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kRdoqWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(levels_bits_kernel, dim3(wgs), dim3(64 * kRdoqWavesPerWg), 0, stream, (const int16_t *)p.d_level, p.n_regions, p.d_class,
                       (const uint32_t *)p.d_nnz, p.d_stat);
    return hipGetLastError();
}

}  // namespace x266
