// rdoq_kernels.hip -- rate-distortion optimised quantisation of 1024-coefficient regions (xRdoQuantRegionsGpu) and the rate estimate of
// a region's levels (xLevelsBitsGpu).  The contract is include/x266hip.h's, the arithmetic x266_rdoq.hpp's, the scan x266_levels.hpp's.
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

namespace x266 {
namespace {

constexpr unsigned kRdoqWavesPerWg = 4;
constexpr unsigned kRdoqRegionBytes = kLevelsRegionWords * 2;
static_assert(sizeof(x266_rdoq_region_t) == 16, "the record is 16 bytes");

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, unsigned o)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), o);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, unsigned o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, (int)o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), (int)o);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t x, unsigned src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)src);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
#pragma unroll
    for (unsigned o = 32; o >= 1; o >>= 1) x += shfl_xor64(x, o);
    return x;
}

__device__ __forceinline__ void rdoq_region_to_lds(const int16_t *src_base, size_t r, unsigned lane, char *slab)
{
    const char *src = reinterpret_cast<const char *>(src_base) + r * kRdoqRegionBytes + lane * 16;
    const v4i a = load16<true>(src), b = load16<true>(src + 1024);
    *reinterpret_cast<v4i *>(slab + lane * 16) = a;
    *reinterpret_cast<v4i *>(slab + 1024 + lane * 16) = b;
}

// the 16 values of the CG whose top-left one is `origin`, rows `n` apart: l[y * 4 + x]
__device__ __forceinline__ void rdoq_cg_from_lds(const char *slab, unsigned origin, unsigned n, int (&l)[16])
{
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const uint2 w = *reinterpret_cast<const uint2 *>(slab + (origin + j * n) * 2);
        l[4 * j + 0] = (int)(int16_t)(w.x & 0xFFFFu);
        l[4 * j + 1] = (int)w.x >> 16;
        l[4 * j + 2] = (int)(int16_t)(w.y & 0xFFFFu);
        l[4 * j + 3] = (int)w.y >> 16;
    }
}
__device__ __forceinline__ void rdoq_cg_to_lds(char *slab, unsigned origin, unsigned n, const int (&l)[16])
{
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        uint2 w;
        w.x = ((uint32_t)l[4 * j + 0] & 0xFFFFu) | ((uint32_t)l[4 * j + 1] << 16);
        w.y = ((uint32_t)l[4 * j + 2] & 0xFFFFu) | ((uint32_t)l[4 * j + 3] << 16);
        *reinterpret_cast<uint2 *>(slab + (origin + j * n) * 2) = w;
    }
}

// What a lane knows of its CG's place: s == 0 (CG 0 of its block), the significance costs of its positions, pos() of its four
// columns and rows.  k = class & 3, n = k + 2.
struct CgPlace {
    bool first;                    // CG 0 of the block
    unsigned sig0_dc, sig1_dc;     // position 0 of the CG: class 0 in CG 0, class 2 elsewhere
    unsigned sig0, sig1;           // the other fifteen: class 1 in CG 0, class 2 elsewhere
    unsigned pos_x[4], pos_y[4];
};
__device__ __forceinline__ CgPlace cg_place(unsigned k, unsigned lane, unsigned origin)
{
    const unsigned n = k + 2u, seg = 1u << (2u * k);
    CgPlace c;
    c.first = (lane & (seg - 1u)) == 0;
    const unsigned dc = c.first ? 0u : 2u, rest = c.first ? 1u : 2u;
    c.sig0_dc = rdoq_sig_bits(dc, 0);
    c.sig1_dc = rdoq_sig_bits(dc, 1);
    c.sig0 = rdoq_sig_bits(rest, 0);
    c.sig1 = rdoq_sig_bits(rest, 1);
    const unsigned in_block = origin & ((1u << (2u * n)) - 1u);             // 4 cgy N + 4 cgx
    const unsigned x0 = in_block & ((1u << n) - 1u), y0 = in_block >> n;
#pragma unroll
    for (unsigned t = 0; t < 4; ++t) {
        c.pos_x[t] = rdoq_last_pos(x0 + t, n);
        c.pos_y[t] = rdoq_last_pos(y0 + t, n);
    }
    return c;
}
// Rlast of scan position i of the lane's CG
__device__ __forceinline__ unsigned last_bits(const CgPlace &c, unsigned i)
{
    return 16u * (c.pos_x[level_scan4(i) & 3u] + c.pos_y[level_scan4(i) >> 2]);
}

// the lanes of a segment of `seg` lanes agree on the highest lane among those with has != 0: -1 when there is none
__device__ __forceinline__ int segment_last_lane(bool has, unsigned lane, unsigned seg)
{
    int best = has ? (int)lane : -1;
    for (unsigned o = 1; o < seg; o <<= 1) {
        const int other = __shfl_xor(best, (int)o);
        best = other > best ? other : best;
    }
    return best;
}

// bits of a lane's CG, given the block's last lane `last` (>= 0) and, in that lane, its last scan position p: rate[i] = R(level) of
// scan position i, any != 0: the CG has a non-zero level
__device__ __forceinline__ unsigned cg_bits(const unsigned (&rate)[16], unsigned any, const CgPlace &c, unsigned lane, int last, unsigned p)
{
    if ((int)lane > last) return 0;
    unsigned sum = 0, at_last = 0;
    const unsigned upto = (int)lane == last ? p : 15u;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {                                     // i is a constant in every copy of the body: no indexed register array
        if (i <= upto) sum += rate[i];
        if (i == p) at_last = last_bits(c, i) - (i ? c.sig1 : c.sig1_dc);
    }
    if ((int)lane == last) return sum + at_last;
    if (c.first) return sum;
    return any ? sum + rdoq_cg_flag_bits(1) : rdoq_cg_flag_bits(0);
}

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
    const unsigned n = k + 2u, seg = 1u << (2u * k), in_seg = lane & (seg - 1u);
    const QuantParams qpar = quant_params(n, q, kRdoqRoundNearest);
    const unsigned origin = level_cg_origin(k, lane);
    int l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) l[i] = 0;
    if (active) rdoq_cg_from_lds(slab, origin, 4u << k, l);
    const CgPlace place = cg_place(k, lane, origin);

    // step 1, in scan order
    unsigned mag[16], dr[16];                                               // by scan position
    uint64_t zero[16];
    unsigned cost_sum = 0, any = 0;
    uint64_t zero_sum = 0;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const int c = l[level_scan4(i)];
        const unsigned a = (unsigned)(c < 0 ? -c : c);
        const unsigned x = rdoq_mul24(a, qpar.f);                           // both below 2^16
        zero[i] = rdoq_dist_zero(x, qpar.qbits);
        const RdoqChoice ch = rdoq_choose(x, qpar.qbits, lambda, i ? place.sig0 : place.sig0_dc, i ? place.sig1 : place.sig1_dc, zero[i]);
        mag[i] = ch.q;
        dr[i] = ch.dr;
        cost_sum += rdoq_cost(ch.dr, lambda);
        zero_sum += zero[i];
        any |= ch.q;
    }
    // step 2
    const uint64_t as_zero = zero_sum + lambda * rdoq_cg_flag_bits(0), as_coded = (uint64_t)cost_sum + lambda * rdoq_cg_flag_bits(1);
    if (!place.first && any && as_zero < as_coded) {
        any = 0;
#pragma unroll
        for (unsigned i = 0; i < 16; ++i) mag[i] = 0;
    }
    // step 3: inclusive scans over the segment of C(s) and of the CG's sum of D(0)
    const uint64_t cg_cost = place.first ? (uint64_t)cost_sum : any ? as_coded : as_zero;
    uint64_t scan_c = cg_cost, scan_z = zero_sum;
    for (unsigned o = 1; o < seg; o <<= 1) {
        const uint64_t tc = shfl_up64(scan_c, o), tz = shfl_up64(scan_z, o);
        if (in_seg >= o) {
            scan_c += tc;
            scan_z += tz;
        }
    }
    const uint64_t block_zero = shfl64(scan_z, lane | (seg - 1u));           // Total(none)
    // Total(p) = base + sum J(q[j < i]) + J(q[i]) - lambda sig1 + lambda Rlast - sum D(0)[j <= i], base = C before + D(0) from this CG on
    const uint64_t base = (scan_c - cg_cost) + (block_zero - (scan_z - zero_sum));
    uint64_t best_total = UINT64_MAX;
    unsigned best_i = 0, run_cost = 0;
    uint64_t run_zero = 0;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const unsigned j = rdoq_cost(dr[i], lambda);
        run_zero += zero[i];
        const uint64_t total = base + run_cost + j + rdoq_mul24(lambda, last_bits(place, i)) - rdoq_mul24(lambda, i ? place.sig1 : place.sig1_dc) - run_zero;
        if (mag[i] && total <= best_total) {
            best_total = total;
            best_i = i;
        }
        run_cost += j;
    }
    uint64_t win_total = best_total;
    unsigned win_lane = lane;
    for (unsigned o = 1; o < seg; o <<= 1) {
        const uint64_t t = shfl_xor64(win_total, o);
        const unsigned w = (unsigned)__shfl_xor((int)win_lane, (int)o);
        if (t < win_total || (t == win_total && w > win_lane)) {
            win_total = t;
            win_lane = w;
        }
    }
    const bool coded = win_total <= block_zero;                             // UINT64_MAX (no candidate in the block) never is; any p wins a tie over none
    const int last = coded ? (int)win_lane : -1;
    // the levels after the last position become 0
    uint64_t dist = 0;
    unsigned count = 0;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const bool keep = (int)lane < last || ((int)lane == last && i <= best_i);
        if (!keep) mag[i] = 0;
        dist += mag[i] ? (uint64_t)(dr[i] & kRdoqDistMask) : zero[i];
        count += mag[i] != 0;
    }
    unsigned rate[16];                                                      // R of the final levels: the chosen level's, or a zero's
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const int c = l[level_scan4(i)];
        rate[i] = mag[i] ? dr[i] >> 20 : (i ? place.sig0 : place.sig0_dc);
        l[level_scan4(i)] = c < 0 ? -(int)mag[i] : (int)mag[i];
    }
    const unsigned lane_bits = cg_bits(rate, any, place, lane, last, best_i);   // here, so that the per-position arrays die before the barrier
    if (active) rdoq_cg_to_lds(slab, origin, 4u << k, l);
    __syncthreads();
    if (!active) return;
    char *dst = reinterpret_cast<char *>(level) + r * kRdoqRegionBytes + lane * 16;
    store16_sc1nt(dst, *reinterpret_cast<const v4i *>(slab + lane * 16));
    store16_sc1nt(dst + 1024, *reinterpret_cast<const v4i *>(slab + 1024 + lane * 16));
    const uint32_t n_nz = wave_sum(count);
    if (nnz && lane == 0) nnz[r] = n_nz;
    if (stat) {
        const uint32_t bits = wave_sum(lane_bits);
        const uint64_t total = wave_sum64(dist);
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

}  // namespace

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
