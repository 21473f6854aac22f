// x266_motion.hpp -- the compact motion stream (xMotionPackGpu, xMotionUnpackGpu): the one host-and-device copy of the Morton map of a
// CTU's blocks, the walk as pack sees it, the level a reader recovers from a head mask, the well-formedness test of a mask and the causal
// predictor.  motion_kernels.hip runs it with a lane per Morton block, the host helpers xMotionWalk, xMotionPredictor and
// xMotionVectorBits (x266hip_abi.hip) and tests/cpp/motion_rules_check.cpp run it as plain C++17 (no HIP).  The geometry, the median and
// the "exactly one" rule are x266_part.hpp's, L is x266_seed.hpp's.  The statement is include/x266hip.h's ("compact motion stream");
// tests/_motion_ref.py restates it in numpy.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/x266hip.h"
#include "x266_part.hpp"

namespace x266 {

constexpr int kMotionWordsPerPart = 4;      // qx, qy, low 16 bits of dx and dy
constexpr int kMotionMaxDiff = 65535;       // |q - P| of two int16 values

// ---- the Morton map of the 8 x 8 blocks of a CTU: bit 2b of i is bit b of x, bit 2b + 1 is bit b of y
X266_HD inline unsigned motion_morton(unsigned x, unsigned y)
{
    return (x & 1u) | (y & 1u) << 1 | (x & 2u) << 1 | (y & 2u) << 2 | (x & 4u) << 2 | (y & 4u) << 3;
}
X266_HD inline unsigned motion_morton_x(unsigned i) { return (i & 1u) | (i >> 1 & 2u) | (i >> 2 & 4u); }
X266_HD inline unsigned motion_morton_y(unsigned i) { return motion_morton_x(i >> 1); }
// the blocks of a node of level k: 4^k consecutive Morton indices from a multiple of 4^k
X266_HD inline unsigned motion_node_blocks(int k) { return 1u << (2 * k); }
X266_HD inline unsigned motion_node_first(unsigned i, int k) { return i & ~(motion_node_blocks(k) - 1u); }

// ---- a CTU of a frame of bw x bh blocks: its first block, which of its Morton blocks exist, which of its nodes are whole
struct MotionCtu {
    int bw, bh, X0, Y0;
};
X266_HD inline int motion_ctus_w(int bw) { return (bw + 7) >> 3; }
X266_HD inline int motion_ctus_h(int bh) { return (bh + 7) >> 3; }
X266_HD inline MotionCtu motion_ctu(int bw, int bh, size_t c)
{
    const size_t cw = (size_t)motion_ctus_w(bw);
    return MotionCtu{bw, bh, (int)(c % cw) * 8, (int)(c / cw) * 8};
}
X266_HD inline int motion_block_x(const MotionCtu &g, unsigned i) { return g.X0 + (int)motion_morton_x(i); }
X266_HD inline int motion_block_y(const MotionCtu &g, unsigned i) { return g.Y0 + (int)motion_morton_y(i); }
X266_HD inline bool motion_block_exists(const MotionCtu &g, unsigned i) { return motion_block_x(g, i) < g.bw && motion_block_y(g, i) < g.bh; }
// the node of level k whose first block is Morton index h (a multiple of 4^k)
X266_HD inline bool motion_node_whole(const MotionCtu &g, unsigned h, int k)
{
    return part_whole(g.bw, g.bh, k, motion_block_x(g, h) >> k, motion_block_y(g, h) >> k);
}
X266_HD inline uint64_t motion_exist_mask(const MotionCtu &g)
{
    uint64_t m = 0;
    for (unsigned i = 0; i < 64; ++i) m |= (uint64_t)motion_block_exists(g, i) << i;
    return m;
}

// ---- the walk as pack sees it, from block i's side: lv[k] = d_level & 3 at the first block of i's node of level k (k = 1..3; lv[0] is not
// looked at).  From level 3 down the first whole node with lv[k] >= k is the partition; level 0 always ends the walk.
X266_HD inline int motion_part_level(const MotionCtu &g, unsigned i, const int (&lv)[4])
{
    for (int k = kPartLevels - 1; k > 0; --k)
        if (motion_node_whole(g, motion_node_first(i, k), k) && lv[k] >= k) return k;
    return 0;
}
// the whole nodes that split on the way to a partition of level k that starts at block i: one flag bit each
X266_HD inline int motion_split_flags(const MotionCtu &g, unsigned i, int k)
{
    int flags = 0;
    for (int j = k + 1; j < kPartLevels; ++j)
        if (motion_node_first(i, j) == i && motion_node_whole(g, i, j)) ++flags;
    return flags;
}

// ---- what a reader recovers from a head mask
X266_HD inline uint64_t motion_bits_below(unsigned i) { return ((uint64_t)1 << i) - 1u; }            // i = 0..63
// the level of head h: the largest k for which h is a multiple of 4^k, the node is whole and no other mask bit lies in (h, h + 4^k)
X266_HD inline int motion_head_level(const MotionCtu &g, uint64_t mask, unsigned h)
{
    for (int k = kPartLevels - 1; k > 0; --k) {
        const unsigned n = motion_node_blocks(k);
        if (motion_node_first(h, k) != h || !motion_node_whole(g, h, k)) continue;
        const uint64_t span = n == 64 ? ~(uint64_t)0 : (motion_bits_below(n) << h);
        if ((mask & span & ~((uint64_t)1 << h)) == 0) return k;
    }
    return 0;
}
// the largest head at or below block i, or -1 if the mask has none there
X266_HD inline int motion_head_of(uint64_t mask, unsigned i)
{
    const uint64_t at_or_below = mask & (motion_bits_below(i) | (uint64_t)1 << i);
    return at_or_below ? 63 - __builtin_clzll(at_or_below) : -1;
}
// block i's part of the well-formedness test: it does not exist, or it lies in [h, h + 4^level(h)) of the largest head h <= i
X266_HD inline bool motion_block_covered(const MotionCtu &g, uint64_t mask, unsigned i)
{
    if (!motion_block_exists(g, i)) return true;
    const int h = motion_head_of(mask, i);
    return h >= 0 && i < (unsigned)h + motion_node_blocks(motion_head_level(g, mask, (unsigned)h));
}
// the part of the test that belongs to no block: bit 0 is set and no bit of a block that does not exist
X266_HD inline bool motion_mask_plausible(uint64_t mask, uint64_t exist) { return (mask & 1u) && !(mask & ~exist); }
inline bool motion_mask_well_formed(const MotionCtu &g, uint64_t mask)
{
    if (!motion_mask_plausible(mask, motion_exist_mask(g))) return false;
    for (unsigned i = 0; i < 64; ++i)
        if (!motion_block_covered(g, mask, i)) return false;
    return true;
}
// the partition of a well-formed mask whose first block is the head with `below` heads before it
X266_HD inline unsigned motion_parts_below(uint64_t mask, unsigned h) { return (unsigned)__builtin_popcountll(mask & motion_bits_below(h)); }

// ---- the causal predictor of the partition of n = 1 << k blocks a side at block (X, Y), from the vectors as they stand in the field (the
// full int16 range, no clamp): A = (X - 1, Y), B = (X, Y - 1), C = (X + n, Y - 1) if that block is inside the frame and precedes the
// partition in coding order -- a CTU above, or this CTU and a lower Morton index --, otherwise (X - 1, Y - 1)
X266_HD inline bool motion_c_right_precedes(int bw, int X, int Y, int n)
{
    const int cx = X + n, cy = Y - 1;
    if (cy < 0 || cx >= bw) return false;
    if ((cy >> 3) < (Y >> 3)) return true;                                  // a CTU row above: a lower raster index, whatever its column
    if ((cx >> 3) > (X >> 3)) return false;                                 // the next CTU of this row
    return motion_morton((unsigned)cx & 7u, (unsigned)cy & 7u) < motion_morton((unsigned)X & 7u, (unsigned)Y & 7u);
}
X266_HD inline PartVec motion_vec_at(const x266_me_result_t *mv, int bw, int bx, int by)
{
    const x266_me_result_t r = mv[(size_t)by * (size_t)bw + (size_t)bx];
    return PartVec{r.mvx, r.mvy};
}
// at(bx, by) is the vector of a block inside the frame; only the spots the rule names are asked for
template <class At>
X266_HD inline PartVec motion_predictor_from(At at, int bw, int X, int Y, int n)
{
    const bool has_a = X > 0, has_b = Y > 0;
    const bool c_right = motion_c_right_precedes(bw, X, Y, n), has_c = c_right || (X > 0 && Y > 0);
    const PartVec zero = {0, 0};
    const PartVec a = has_a ? at(X - 1, Y) : zero, b = has_b ? at(X, Y - 1) : zero;
    const PartVec c = c_right ? at(X + n, Y - 1) : (has_c ? at(X - 1, Y - 1) : zero);
    return part_predict3(has_a, a, has_b, b, has_c, c);
}
X266_HD inline PartVec motion_predictor(const x266_me_result_t *mv, int bw, int X, int Y, int n)
{
    return motion_predictor_from([=](int bx, int by) { return motion_vec_at(mv, bw, bx, by); }, bw, X, Y, n);
}

// ---- a partition's share of `bits`: its flag, the two differences, and the whole nodes that split above it
X266_HD inline uint32_t motion_part_bits(const MotionCtu &g, unsigned h, int k, int dx, int dy)
{
    return (uint32_t)((k > 0 ? 1 : 0) + seed_code_length(dx) + seed_code_length(dy) + motion_split_flags(g, h, k));
}
X266_HD inline uint32_t motion_abs(int d) { return (uint32_t)(d < 0 ? -d : d); }

}  // namespace x266
