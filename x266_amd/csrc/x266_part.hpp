// x266_part.hpp -- the inter partition decision (xInterPartitionDecideGpu): the one copy of its arithmetic that is not sample work --
// the clamp of an input vector and of a candidate, the node geometry and the d_nodes offsets, the predictor of a node and the rate R.
// partition_kernels.hip runs it on the device, x266_args.hpp takes the extents from it on the host and tests/cpp/partition_rules_check.cpp
// runs it as plain C++17 (no HIP).  L is x266_seed.hpp's.  The statement is include/x266hip.h's ("inter partition decision");
// tests/_partition_ref.py restates it in numpy.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/x266hip.h"
#include "x266_seed.hpp"

namespace x266 {

constexpr int kPartLevels = 4;              // node sides of 8, 16, 32 and 64 samples
constexpr int kPartMaxRange = 1;            // r: 0..1
constexpr int kPartClamp = 32766;           // in(): what an input component is clamped to

struct PartVec {
    int x, y;
};

X266_HD inline int part_clamp_in(int c) { return c < -kPartClamp ? -kPartClamp : (c > kPartClamp ? kPartClamp : c); }
// a candidate component: W(child) + d, held to what an x266_me_result_t can say
X266_HD inline int part_clamp_cand(int c) { return c < -32768 ? -32768 : (c > 32767 ? 32767 : c); }

// in(bx, by): the clamped input vector of a block inside the frame
X266_HD inline PartVec part_in(const x266_me_result_t *mv, int bw, int bx, int by)
{
    const x266_me_result_t r = mv[(size_t)by * (size_t)bw + (size_t)bx];
    return PartVec{part_clamp_in(r.mvx), part_clamp_in(r.mvy)};
}

// ---- geometry: level k has nodes of 1 << k blocks a side on the grid anchored at (0, 0); bw, bh are the frame's sides in blocks
X266_HD inline int part_whole_w(int bw, int k) { return bw >> k; }
X266_HD inline int part_whole_h(int bh, int k) { return bh >> k; }
X266_HD inline bool part_whole(int bw, int bh, int k, int nx, int ny) { return nx < part_whole_w(bw, k) && ny < part_whole_h(bh, k); }
// a node exists if its first block lies inside the frame
X266_HD inline bool part_exists(int bw, int bh, int k, int nx, int ny) { return (nx << k) < bw && (ny << k) < bh; }
inline size_t part_whole_nodes(int bw, int bh, int k) { return (size_t)part_whole_w(bw, k) * (size_t)part_whole_h(bh, k); }
// d_nodes: level 1 first, then 2, then 3, each the raster of its whole nodes
X266_HD inline size_t part_nodes_offset(int bw, int bh, int k)
{
    size_t at = 0;
    for (int j = 1; j < k; ++j) at += (size_t)part_whole_w(bw, j) * (size_t)part_whole_h(bh, j);
    return at;
}
inline size_t part_nodes_total(int bw, int bh) { return part_nodes_offset(bw, bh, kPartLevels); }

// ---- the predictor of the node of n blocks a side at block (X, Y), from the input field alone
X266_HD inline int part_median3(int a, int b, int c)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
}
// P from the three spots, one outside the frame handed in as (0, 0): exactly one inside -> that one; otherwise the component-wise median.
// Shared with the causal predictor of the motion stream (x266_motion.hpp).
X266_HD inline PartVec part_predict3(bool has_a, const PartVec &a, bool has_b, const PartVec &b, bool has_c, const PartVec &c)
{
    if ((int)has_a + (int)has_b + (int)has_c == 1) return has_a ? a : (has_b ? b : c);
    return PartVec{part_median3(a.x, b.x, c.x), part_median3(a.y, b.y, c.y)};
}
X266_HD inline PartVec part_predictor(const x266_me_result_t *mv, int bw, int X, int Y, int n)
{                                                                           // (X, Y) inside the frame: no neighbour lies below it
    const bool has_a = X > 0, has_b = Y > 0;
    const bool c_right = Y > 0 && X + n < bw, has_c = c_right || (X > 0 && Y > 0);
    const PartVec zero = {0, 0};
    const PartVec a = has_a ? part_in(mv, bw, X - 1, Y) : zero, b = has_b ? part_in(mv, bw, X, Y - 1) : zero;
    const PartVec c = c_right ? part_in(mv, bw, X + n, Y - 1) : (has_c ? part_in(mv, bw, X - 1, Y - 1) : zero);
    return part_predict3(has_a, a, has_b, b, has_c, c);
}

// ---- R(k, q) = (k > 0) + L(qx - Px) + L(qy - Py), at most 67, and what it costs: (lambda_q4 * R) >> 4
X266_HD inline uint32_t part_rate(int k, int qx, int qy, const PartVec &p)
{
    return (uint32_t)((k > 0 ? 1 : 0) + seed_code_length(qx - p.x) + seed_code_length(qy - p.y));
}
X266_HD inline uint32_t part_rate_cost(int lambda_q4, uint32_t bits) { return ((uint32_t)lambda_q4 * bits) >> 4; }

// ---- the walk of a node's candidates: children TL, TR, BL, BR; per child dy = -r..r ascending, then dx = -r..r ascending
X266_HD inline int part_walk_length(int r) { return 4 * (2 * r + 1) * (2 * r + 1); }
struct PartStep {
    int child, dx, dy;
};
X266_HD inline PartStep part_walk_step(int c, int r)
{
    const int span = 2 * r + 1, child = c / (span * span), rem = c - child * span * span, dyi = rem / span;
    return PartStep{child, rem - dyi * span - r, dyi - r};
}

}  // namespace x266
