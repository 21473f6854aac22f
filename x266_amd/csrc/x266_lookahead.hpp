// x266_lookahead.hpp -- the lookahead: the one copy of the arithmetic behind xLaDownscaleGpu, xLaIntraCostsGpu, xLaFrameCostGpu,
// xLaPropagateGpu, xLaTreeQpGpu (lookahead_kernels.hip) and the host call xSceneCutFromTotals.  The statement is include/x266hip.h's
// ("lookahead"); tests/_la_ref.py restates it in numpy.  L(e), the rounding of a mean offset and the clamp of a region's qp are the
// source analysis' (x266_aq.hpp), used, not copied.
#pragma once

#include "../../include/x266hip.h"
#include "x266_aq.hpp"

namespace x266 {

constexpr unsigned kLaTotalsThreads = 1024;        // lanes of the totals' one workgroup
constexpr unsigned kLaTotalsChunk = 2048;          // blocks it takes per full step (xLaTotalsChunk): two per lane
// candidate c = 0..3 in the order they are tried: planar, DC, horizontal, vertical, by the library's mode numbers
__host__ __device__ inline unsigned la_mode_number(int c) { return c == 0 ? 0u : c == 1 ? 1u : c == 2 ? 10u : 26u; }

// ---- 1. the 2x2 box ----------------------------------------------------------------------------------------------------------------------
// four samples of an upper and of a lower row (a dword each) -> the two box means in the two 16-bit halves; a half holds at most 1022
__host__ __device__ inline uint32_t la_box_pairs(uint32_t upper, uint32_t lower)
{
    const uint32_t m = 0x00FF00FFu;
    const uint32_t s = (upper & m) + ((upper >> 8) & m) + (lower & m) + ((lower >> 8) & m) + 0x00020002u;
    return (s >> 2) & m;
}
// eight samples of each row (dwords u0 u1 / l0 l1) -> four output samples in one dword
__host__ __device__ inline uint32_t la_box_luma(uint32_t u0, uint32_t u1, uint32_t l0, uint32_t l1)
{
    const uint32_t a = la_box_pairs(u0, l0), b = la_box_pairs(u1, l1);
    return (a & 0xFFu) | ((a >> 8) & 0xFF00u) | ((b & 0xFFu) << 16) | ((b & 0xFF0000u) << 8);
}
// two (U, V) pairs of each row -> one (U, V) pair in the low 16 bits: U is the even bytes, V the odd ones
__host__ __device__ inline uint32_t la_box_uv(uint32_t upper, uint32_t lower)
{
    const uint32_t m = 0x00FF00FFu;
    const uint32_t u = (upper & m) + (lower & m), v = ((upper >> 8) & m) + ((lower >> 8) & m);
    return ((((u & 0xFFFFu) + (u >> 16) + 2u) >> 2) & 0xFFu) | (((((v & 0xFFFFu) + (v >> 16) + 2u) >> 2) & 0xFFu) << 8);
}
// four pairs of each row (dwords u0 u1 / l0 l1) -> two output pairs in one dword
__host__ __device__ inline uint32_t la_box_chroma(uint32_t u0, uint32_t u1, uint32_t l0, uint32_t l1)
{
    return la_box_uv(u0, l0) | (la_box_uv(u1, l1) << 16);
}

// ---- 2. open-loop intra costs of a lowres 8x8 block ---------------------------------------------------------------------------------------
// byte offset of luma sample (x, y) in a tiled frame of tiles_w tiles per row
__host__ __device__ inline size_t la_luma_at(unsigned x, unsigned y, unsigned tiles_w)
{
    return ((size_t)(y >> 4) * tiles_w + (x >> 4)) * 512u + (y & 15u) * 16u + (x & 15u);
}
// What row y of the block at (x0, y0) needs of its neighbours: top[0..8], left[y], left[8] and the sum of left[0..7].  `luma` is the
// lowres frame's first byte; w, h its sides.  Every lane of a block reads the same few bytes: they come from the cache.
struct LaEdge {
    int top[9], left_y, bl, sum_left;
};
__host__ __device__ inline LaEdge la_edge(const uint8_t *luma, unsigned x0, unsigned y0, unsigned y, unsigned w, unsigned h)
{
    LaEdge e;
    const unsigned tiles_w = w >> 4;
    if (x0 == 0 && y0 == 0) {
        for (int i = 0; i < 9; ++i) e.top[i] = 128;
        e.left_y = e.bl = 128;
        e.sum_left = 8 * 128;
        return e;
    }
    if (y0 > 0) {
        for (unsigned i = 0; i < 9; ++i) e.top[i] = luma[la_luma_at(x0 + i < w ? x0 + i : w - 1, y0 - 1, tiles_w)];
    } else {
        const int l0 = luma[la_luma_at(x0 - 1, y0, tiles_w)];
        for (int i = 0; i < 9; ++i) e.top[i] = l0;
    }
    if (x0 > 0) {
        e.left_y = luma[la_luma_at(x0 - 1, y0 + y, tiles_w)];
        e.bl = luma[la_luma_at(x0 - 1, y0 + 8 < h ? y0 + 8 : h - 1, tiles_w)];
        e.sum_left = 0;
        for (unsigned i = 0; i < 8; ++i) e.sum_left += luma[la_luma_at(x0 - 1, y0 + i, tiles_w)];
    } else {
        e.left_y = e.bl = e.top[0];
        e.sum_left = 8 * e.top[0];
    }
    return e;
}
// row y of candidate c
__host__ __device__ inline void la_pred_row(int c, int y, const LaEdge &e, int pred[8])
{
    int sum_top = 0;
    for (int x = 0; x < 8; ++x) sum_top += e.top[x];
    for (int x = 0; x < 8; ++x)
        pred[x] = c == 0   ? ((7 - x) * e.left_y + (x + 1) * e.top[8] + (7 - y) * e.top[x] + (y + 1) * e.bl + 8) >> 4
                  : c == 1 ? (sum_top + e.sum_left + 8) >> 4
                  : c == 2 ? e.left_y
                           : e.top[x];
}
// the 8-point Hadamard transform in place (natural order; the sum of magnitudes does not depend on the order)
__host__ __device__ inline void la_hadamard8(int v[8])
{
#pragma unroll
    for (int d = 1; d < 8; d <<= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (!(i & d)) {
                const int a = v[i], b = v[i | d];
                v[i] = a + b;
                v[i | d] = a - b;
            }
}
__host__ __device__ inline uint32_t la_satd_round(uint32_t sum_abs) { return (sum_abs + 2u) >> 2; }

// ---- 3. a block's decision ----------------------------------------------------------------------------------------------------------------
// l0 / l1: the lists' records, looked at when has0 / has1; ties go to list 0, then list 1, then intra
__host__ __device__ inline x266_la_block_t la_decide(uint32_t intra, unsigned mode, bool has0, x266_me_result_t l0, bool has1, x266_me_result_t l1,
                                                     uint32_t intra_penalty)
{
    x266_la_block_t r;
    x266_me_result_t best = l0;
    r.kind = has0 ? 1 : 0;
    if (has1 && (!has0 || l1.cost < best.cost)) {
        best = l1;
        r.kind = 2;
    }
    const uint32_t ci = intra + intra_penalty;
    if (r.kind == 0 || ci < best.cost) {
        best.mvx = best.mvy = 0;
        best.cost = ci;
        r.kind = 0;
    }
    r.cost = best.cost;
    r.intra = intra;
    r.mvx = best.mvx;
    r.mvy = best.mvy;
    r.mode = (uint8_t)mode;
    r.reserved = 0;
    return r;
}

// ---- 4. the scene cut (host) --------------------------------------------------------------------------------------------------------------
inline int64_t la_scene_cut_bias(int threshold_q8, int g, int min_keyint, int max_keyint)
{
    const int64_t tmax = (int64_t)threshold_q8 << 8, tmin = tmax >> 2;
    if (4 * (int64_t)g <= min_keyint) return tmin >> 2;
    if (g <= min_keyint) return tmin * g / min_keyint;
    if (max_keyint == min_keyint) return tmax;
    return tmin + (tmax - tmin) * ((int64_t)g - min_keyint) / ((int64_t)max_keyint - min_keyint);
}
inline int la_scene_cut(const int64_t total[8], int threshold_q8, int g, int min_keyint, int max_keyint)
{
    const int64_t bias = la_scene_cut_bias(threshold_q8, g, min_keyint, max_keyint);
    if (bias >= 65536) return 1;                                            // g far past max_keyint: the right side is <= 0, and its product need not be formed
    return total[0] * 65536 >= (65536 - bias) * total[1] ? 1 : 0;           // totals are held to 2^40: both products fit
}

// ---- 5. the propagation tree --------------------------------------------------------------------------------------------------------------
// what a block hands on; intra != 0
__host__ __device__ inline uint64_t la_amount(uint32_t cost, uint32_t intra, uint64_t prop)
{
    const uint64_t q = prop < 0xFFFFFFFFull ? prop : 0xFFFFFFFFull;
    const uint32_t inter = cost < intra ? cost : intra;
    return (((uint64_t)intra + q) * (uint64_t)(intra - inter)) / intra;
}
// The four targets of block (bx, by) with vector (mvx, mvy): index[k] is the target's block index or -1 when it lies outside the grid or
// its weight is 0, share[k] what it receives.
struct LaTargets {
    long long index[4];
    uint64_t share[4];
};
__host__ __device__ inline LaTargets la_targets(int bx, int by, int mvx, int mvy, int blocks_w, int blocks_h, uint64_t amount)
{
    const int px = 8 * bx + mvx, py = 8 * by + mvy;
    const int X = px >> 3, Y = py >> 3, dx = px & 7, dy = py & 7;           // the shift is arithmetic: floor
    LaTargets t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tx = X + (k & 1), ty = Y + (k >> 1);
        const int w = ((k & 1) ? dx : 8 - dx) * ((k >> 1) ? dy : 8 - dy);
        const bool in = w > 0 && tx >= 0 && tx < blocks_w && ty >= 0 && ty < blocks_h;
        t.index[k] = in ? (long long)ty * blocks_w + tx : -1;
        t.share[k] = (amount * (uint64_t)w + 32u) >> 6;
    }
    return t;
}

// ---- 6. a tile's offset from what it handed on --------------------------------------------------------------------------------------------
__host__ __device__ inline int la_gain_q8(uint32_t intra, uint64_t prop, int strength_q8)
{
    if (intra == 0) return 0;
    const uint64_t room = 0xFFFFFFFFull - intra;
    const uint32_t p = (uint32_t)(prop < room ? prop : room);
    return (strength_q8 * (int)(aq_log2_q8(intra + p) - aq_log2_q8(intra))) >> 8;   // the difference is 0..8191: below 2^23
}
__host__ __device__ inline int la_tree_offset_q8(int aq_offset_q8, int gain_q8)
{
    const int off = aq_offset_q8 - gain_q8;
    return off < -kAqOffsetMaxQ8 ? -kAqOffsetMaxQ8 : off > kAqOffsetMaxQ8 ? kAqOffsetMaxQ8 : off;
}

}  // namespace x266
