// x266_seed.hpp -- the seeded SATD search (xSatd8x8SeededSearchGpu): the one copy of its arithmetic -- the seed grid, the clamp of a
// seed, the ordered centre list of a cell, the walk of the candidates and the vector cost L.  seeded_search_kernels.hip runs it on the
// device, x266_args.hpp takes the grid and the scalar ranges from it on the host (plain C++17 there: no HIP).  The statement is
// include/x266hip.h's ("hierarchical motion search"); tests/_seeded_ref.py restates it in numpy.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/x266hip.h"

#if defined(__HIPCC__)
#define X266_HD __host__ __device__
#else
#define X266_HD
#endif

namespace x266 {

constexpr int kSeedMaxRange = 8;            // r: 0..8
constexpr int kSeedMaxCentres = 6;          // own, (0, 0), left, top, right, bottom
constexpr int kSeedCentreBits = 31;         // the `centres` mask: bits 0..4 add centres 1..5
constexpr int kSeedClamp = 8183;            // 8183 + 8 = 8191: what the quarter-sample refinement takes unclamped

struct SeedVec {
    int x, y;
};

// the seed grid: one cell per 8x8 block (seed_scale 0) or per 16x16 tile (seed_scale 1)
X266_HD inline int seed_grid_w(int width, int seed_scale) { return width >> (3 + seed_scale); }
X266_HD inline int seed_grid_h(int height, int seed_scale) { return height >> (3 + seed_scale); }
inline size_t seed_cells(int width, int height, int seed_scale) { return (size_t)seed_grid_w(width, seed_scale) * (size_t)seed_grid_h(height, seed_scale); }

// S = clamp(seed << seed_scale, -8183, 8183), in 32 bits: -32768 and 32767 are defined
X266_HD inline int seed_clamp(int seed, int seed_scale)
{
    const int s = seed * (1 << seed_scale);
    return s < -kSeedClamp ? -kSeedClamp : (s > kSeedClamp ? kSeedClamp : s);
}
X266_HD inline SeedVec seed_at(const x266_me_result_t *seed, int grid_w, int sx, int sy, int seed_scale)
{
    const x266_me_result_t r = seed[(size_t)sy * (size_t)grid_w + (size_t)sx];
    return SeedVec{seed_clamp(r.mvx, seed_scale), seed_clamp(r.mvy, seed_scale)};
}

// The ordered centre list of cell (sx, sy): own always; (0, 0), left, top, right, bottom when their bit is set; a neighbour outside the
// grid is skipped, not substituted.  Returns the number of centres, 1..6; c[0] is the predictor P.
X266_HD inline int seed_centre_list(const x266_me_result_t *seed, int grid_w, int grid_h, int sx, int sy, int seed_scale, int centres, SeedVec (&c)[kSeedMaxCentres])
{
    int n = 0;
    c[n++] = seed_at(seed, grid_w, sx, sy, seed_scale);
    if (centres & 1) c[n++] = SeedVec{0, 0};
    if ((centres & 2) && sx > 0) c[n++] = seed_at(seed, grid_w, sx - 1, sy, seed_scale);
    if ((centres & 4) && sy > 0) c[n++] = seed_at(seed, grid_w, sx, sy - 1, seed_scale);
    if ((centres & 8) && sx + 1 < grid_w) c[n++] = seed_at(seed, grid_w, sx + 1, sy, seed_scale);
    if ((centres & 16) && sy + 1 < grid_h) c[n++] = seed_at(seed, grid_w, sx, sy + 1, seed_scale);
    return n;
}

// The walk: centres in list order, per centre dy = -r..r ascending, then dx = -r..r ascending.  Walk index t -> (centre, dx + r, dy + r).
struct SeedStep {
    int centre, dxi, dyi;
};
X266_HD inline int seed_walk_length(int n_centres, int r) { return n_centres * (2 * r + 1) * (2 * r + 1); }
X266_HD inline SeedStep seed_walk_step(int t, int r)
{
    const int span = 2 * r + 1, centre = t / (span * span), rem = t - centre * span * span, dyi = rem / span;
    return SeedStep{centre, rem - dyi * span, dyi};
}

// L(d), the length of d as a signed Exp-Golomb code: k = 2|d| - (d > 0), L = 2 floor(log2(k + 1)) + 1.  |d| <= 16382: L <= 29.
X266_HD inline int seed_code_length(int d)
{
    const unsigned k = 2u * (unsigned)(d < 0 ? -d : d) - (d > 0 ? 1u : 0u);
    return 2 * (31 - __builtin_clz(k + 1u)) + 1;
}
// what the vector costs beside the SATD: (lambda_q4 * (L(vx - Px) + L(vy - Py))) >> 4, at most 65535 * 58 >> 4
X266_HD inline uint32_t seed_vector_cost(int lambda_q4, int vx, int vy, const SeedVec &p)
{
    return ((uint32_t)lambda_q4 * (uint32_t)(seed_code_length(vx - p.x) + seed_code_length(vy - p.y))) >> 4;
}

}  // namespace x266
