// x266_rdoq.hpp -- rate-distortion optimised quantisation and the level rate estimate: the one copy of the rate tables, of the rate
// functions, of the per-coefficient candidate costs and of the last-position cost that the kernels of rdoq_kernels.hip and the host
// helpers xLevelBits, xLastPosBits and xCgFlagBits share.  The statement is include/x266hip.h's (xRdoQuantRegionsGpu ...); f and
// qbits are x266_quant.hpp's QuantParams, the scan and the CG origins x266_levels.hpp's.
//
// Rate is in 1/16 bit, distortion in 1/65536 of a squared level, lambda in 1/4096 of a squared level per bit: J = D + lambda * R.
// What follows from the contract's ranges, and what the kernels rely on -- where 32 bits are used, this is why they are enough:
//   * a = |c| <= 32768 and f < 2^15 (the largest of the six is the first), so x = a * f < 2^30, and both factors fit the 24-bit multiply;
//   * h = (x + half) >> qbits <= 13108, so rem() sees at most 13105 and R(l) <= 36 + 16 + 24 + 22 + 16 * 30 = 578 for every level
//     the optimisation can emit; an arbitrary int16 level (xLevelsBitsGpu) has |l| <= 32768 and R <= 610, and 1024 of them with
//     the last-position cost (at most 16 * 24) and 63 CG flags stay below 2^20: `bits` is a uint32 with room to spare;
//   * for a CANDIDATE level (h, h - 1, or 0 when h <= 2) err < 2.5 * 2^qbits, so e <= 641 and D <= 410881 < 2^19; with
//     lambda * R <= 8192 * 578 < 2^23 a candidate's J is below 2^24, the 16 of a CG below 2^28: 32-bit arithmetic is exact for
//     every J of a kept level, and e * e and lambda * R are 24-bit multiplies.  D and R of the chosen level travel in one dword
//     (D in bits 0..19, R above);
//   * D(0) of an ARBITRARY coefficient is not bounded that way: e = (x + ...) >> (qbits - 8) reaches 2^22 at qbits = 16, D(0) 2^44,
//     the sum over a region 2^54.  Every sum that holds a D(0) -- Jz, C(s), the prefix and suffix sums of step 3, Total, dist -- is
//     64 bits wide.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_levels.hpp"
#include "x266_quant.hpp"

namespace x266 {

constexpr unsigned kRdoqLambdaMax = 8192;
constexpr unsigned kRdoqSignBits = 16;
constexpr unsigned kRdoqRoundNearest = 256;        // the `rounding` that makes QuantParams::offset = 1 << (qbits - 1)

// position class: 0 at DC, 1 elsewhere in CG 0, 2 otherwise
__host__ __device__ constexpr unsigned rdoq_sig_bits(unsigned pos_class, unsigned significant)
{
    return pos_class == 0 ? (significant ? 10u : 24u) : pos_class == 1 ? (significant ? 22u : 12u) : (significant ? 36u : 6u);
}
__host__ __device__ constexpr unsigned rdoq_gt1_bits(unsigned greater) { return greater ? 24u : 10u; }
__host__ __device__ constexpr unsigned rdoq_gt2_bits(unsigned greater) { return greater ? 22u : 11u; }
__host__ __device__ constexpr unsigned rdoq_cg_flag_bits(unsigned coded) { return coded ? 26u : 9u; }

// a * b for factors below 2^24 (every use below is one, by the bounds above): the masks change no value and tell the compiler so,
// which then picks the full-rate 24-bit multiply instead of the quarter-rate 32-bit one
__host__ __device__ inline unsigned rdoq_mul24(unsigned a, unsigned b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }

// floor(log2 t), t >= 1
__host__ __device__ inline unsigned rdoq_ilog2(unsigned t) { return 31u - (unsigned)__builtin_clz(t); }

// the remainder r >= 0 of a level above 2, in bits (not sixteenths)
__host__ __device__ inline unsigned rdoq_rem(unsigned r) { return r < 3u ? r + 1u : 4u + 2u * rdoq_ilog2(r < 3u ? 1u : r - 2u); }

// R(l) of a level magnitude l, given the two significance costs of its position class
__host__ __device__ inline unsigned rdoq_level_bits(unsigned l, unsigned sig0, unsigned sig1)
{
    const unsigned base = sig1 + kRdoqSignBits;                             // straight-line: selects, no divergent branches in a wave
    const unsigned above = base + rdoq_gt1_bits(1) + rdoq_gt2_bits(1) + 16u * rdoq_rem(l < 3u ? 0u : l - 3u);
    return l == 0 ? sig0 : l == 1 ? base + rdoq_gt1_bits(0) : l == 2 ? base + rdoq_gt1_bits(1) + rdoq_gt2_bits(0) : above;
}

// pos(t) of one coordinate t < N = 1 << n of the last position; Rlast(u, v) = 16 * (pos(u) + pos(v))
__host__ __device__ inline unsigned rdoq_last_pos(unsigned t, unsigned n)
{
    unsigned g = t;
    if (t >= 4u) {
        const unsigned k = rdoq_ilog2(t);
        g = 2u * k + ((t >> (k - 1u)) & 1u);
    }
    const unsigned prefix = g + 1u < 2u * n - 1u ? g + 1u : 2u * n - 1u;
    return prefix + (g >= 4u ? (g >> 1) - 1u : 0u);
}

// e of a level magnitude l for x = |c| * f: |x - (l << qbits)| in 1/256 of a level, rounded
__host__ __device__ inline unsigned rdoq_err(unsigned x, unsigned l, unsigned qbits)
{
    const unsigned y = l << qbits;
    const unsigned err = x > y ? x - y : y - x;
    return (err + (1u << (qbits - 9u))) >> (qbits - 8u);
}
// D of a candidate level: e <= 641
__host__ __device__ inline unsigned rdoq_dist_candidate(unsigned x, unsigned l, unsigned qbits)
{
    const unsigned e = rdoq_err(x, l, qbits);
    return rdoq_mul24(e, e);
}
// D(0) of any coefficient
__host__ __device__ inline uint64_t rdoq_dist_zero(unsigned x, unsigned qbits)
{
    const uint64_t e = rdoq_err(x, 0u, qbits) & 0xFFFFFFu;                  // below 2^23: the 24-bit multiply pair
    return e * e;
}

// Step 1 for one coefficient; d0 = rdoq_dist_zero(x, qbits), which the caller needs anyway and which is the candidate 0's D when
// h <= 2 (then below 2^19).  dr = D(q) | R(q) << 20 of the chosen magnitude q.
struct RdoqChoice {
    unsigned q, dr;
};
constexpr unsigned kRdoqDistMask = (1u << 20) - 1u;
__host__ __device__ inline unsigned rdoq_cost(unsigned dr, unsigned lambda) { return (dr & kRdoqDistMask) + rdoq_mul24(lambda, dr >> 20); }

__host__ __device__ inline RdoqChoice rdoq_choose(unsigned x, unsigned qbits, unsigned lambda, unsigned sig0, unsigned sig1, uint64_t d0)
{
    const unsigned h = (x + (1u << (qbits - 1u))) >> qbits;
    RdoqChoice best = {h, rdoq_dist_candidate(x, h, qbits) | rdoq_level_bits(h, sig0, sig1) << 20};
    unsigned cost = rdoq_cost(best.dr, lambda);
    // h - 1 if h >= 1 (at h = 0 the "candidate" is h itself again and changes nothing); on a tie the smaller level wins
    const unsigned below = h ? h - 1u : 0u;
    const unsigned dr1 = rdoq_dist_candidate(x, below, qbits) | rdoq_level_bits(below, sig0, sig1) << 20, j1 = rdoq_cost(dr1, lambda);
    if (j1 <= cost) {
        best = {below, dr1};
        cost = j1;
    }
    // 0 if h <= 2: at h = 1 it is h - 1, at h = 0 it is h, so only h = 2 adds a candidate (d0 is its D, below 2^19 there)
    const unsigned dr0 = ((unsigned)d0 & kRdoqDistMask) | sig0 << 20;
    if (h == 2u && rdoq_cost(dr0, lambda) <= cost) best = {0u, dr0};
    return best;
}

}  // namespace x266
