// x266_rdoq_blocks.hpp -- the per-wave pieces of rdoq_kernels.hip: a region between memory, its LDS slab and the CG-per-lane
// arrangement, a lane's place in its block, the three RDOQ steps on a lane's CG, and the rate of a CG's final levels.  Shared by the
// kernels of xRdoQuantRegionsGpu, xLevelsBitsGpu and xTransformDecideCtuTilesGpu: the decision runs rdoq_steps on each candidate's
// coefficients, so "its levels and statistics are xRdoQuantRegionsGpu's" holds by construction.  The arithmetic is x266_rdoq.hpp's.
//
// Lane g = CG bit g (the compact level stream's arrangement): a block of N = 4 << k is a segment of (N / 4)^2 = 1, 4, 16 or 64
// consecutive lanes whose order is the block's CG scan.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_levels.hpp"
#include "x266_quant.hpp"
#include "x266_rdoq.hpp"

namespace x266 {

constexpr unsigned kRdoqWavesPerWg = 4;
constexpr unsigned kRdoqRegionBytes = kLevelsRegionWords * 2;
static_assert(sizeof(x266_rdoq_region_t) == 16, "the record is 16 bytes");

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

// What a lane's CG adds to its region's record after the three steps
struct RdoqLane {
    uint64_t dist;                 // sum of D(final level) over the CG
    unsigned bits, count;          // the CG's share of the region's bits; its non-zero levels
};

// The three steps on a lane's CG of a region of blocks of N = 4 << k: l[y * 4 + x] holds the CG's coefficients on entry and its
// levels on return.  Every lane of the wave calls it (steps 3's scans cross the block's lanes); lane, k, origin = level_cg_origin(k,
// lane) and place = cg_place(k, lane, origin) describe the CG, qpar and lambda the region.
//   step 1  lane-local: 16 coefficients, two or three candidates each; the lane keeps q, D(q) | R(q) << 20 and D(0) per position
//   step 2  one 64-bit comparison per lane
//   step 3  an inclusive scan of (C(s), sum D(0)) over the segment's lanes (__shfl_up, 64-bit pairs), each lane's at most 16
//           candidate totals in scan order with "<=" (the later position wins a tie), then the minimum of (Total, lane) across the
//           segment by butterfly (__shfl_xor; the higher lane wins a tie).  Every lane of the segment ends with the same winner.
__device__ __forceinline__ RdoqLane rdoq_steps(int (&l)[16], unsigned k, unsigned lane, const CgPlace &place, const QuantParams &qpar, unsigned lambda)
{
    const unsigned seg = 1u << (2u * k), in_seg = lane & (seg - 1u);
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
    RdoqLane out = {0, 0, 0};
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const bool keep = (int)lane < last || ((int)lane == last && i <= best_i);
        if (!keep) mag[i] = 0;
        out.dist += mag[i] ? (uint64_t)(dr[i] & kRdoqDistMask) : zero[i];
        out.count += mag[i] != 0;
    }
    unsigned rate[16];                                                      // R of the final levels: the chosen level's, or a zero's
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) {
        const int c = l[level_scan4(i)];
        rate[i] = mag[i] ? dr[i] >> 20 : (i ? place.sig0 : place.sig0_dc);
        l[level_scan4(i)] = c < 0 ? -(int)mag[i] : (int)mag[i];
    }
    out.bits = cg_bits(rate, any, place, lane, last, best_i);
    return out;
}

}  // namespace x266
