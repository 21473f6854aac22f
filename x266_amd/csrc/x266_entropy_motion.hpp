// x266_entropy_motion.hpp -- the entropy coder of the motion stream: the one copy of the context layout, of the default table and of a
// CTU's syntax that the kernels of entropy_motion_kernels.hip (xEntropyEncodeMvGpu, xEntropyDecodeMvGpu) and the host helpers
// xEntropyMvDefaultInit, xEntropyEncodeMvCtu and xEntropyDecodeMvCtu share.  The statement is include/x266hip.h's ("the entropy
// coder of the motion stream"); the coder is x266_entropy.hpp's, used as it is; geometry, Morton map, level-from-mask rule and the bits
// of a partition are x266_motion.hpp's.  Plain C++17 for the host-only driver (tests/cpp/entropy_motion_rules_check.cpp).
//
// The walk needs no recursion on either side.  Encoder: the partitions come in ascending Morton index of their heads, and every node of
// the quadtree has a first block that is the head of the first partition inside it -- so the split bins of the nodes above a partition
// are due exactly at the head that is their first block, from level 3 down, and then the partition's own "not split" bin.  Decoder: a
// cursor i over the Morton indices; where it stands a node of every level that i is a multiple of begins, from the largest down.
// Every loop is bounded by the syntax: 64 cursor positions, 3 levels, 14 prefix ones, 15 suffix bits.
#pragma once

#include <cstdint>

#include "x266_entropy.hpp"
#include "x266_motion.hpp"

namespace x266 {

constexpr unsigned kEntropyMotionContexts = X266_ENTROPY_MOTION_CONTEXTS;
constexpr unsigned kEntropyMotionMaxBytes = X266_ENTROPY_MOTION_MAX_BYTES;
constexpr unsigned kMotionCtuWords = 256;                                   // 64 partitions of 4 words: the payload of a CTU at most
static_assert(kEntropyMotionContexts == 7, "split of level 1, 2, 3; nz x, y; gt1 x, y");
static_assert(kEntropyMotionMaxBytes % 16 == 0, "the staging slabs hold whole 16-byte chunks");

// split of level k is context k - 1; nz and gt1 take the component, 0 = x
constexpr unsigned kMotionCtxSplit = 0, kMotionCtxNz = 3, kMotionCtxGt1 = 5;
constexpr unsigned kMotionMaxPrefix = 14;                                   // ones of the Exp-Golomb prefix: k - 1 with k <= 15

struct EntropyMotionInit {
    uint16_t p[kEntropyMotionContexts];
};
// the estimate this syntax mirrors (xMotionVectorBits, one bit per flag) has no skew
constexpr EntropyMotionInit kEntropyMotionDefault = {{1024, 1024, 1024, 1024, 1024, 1024, 1024}};

// ---- one component of a difference, |d| <= 65535 ------------------------------------------------------------------------------------------
X266_HD inline void entropy_motion_enc_diff(EntropyEnc &e, uint16_t *ctx, unsigned comp, int d)
{
    const unsigned a = motion_abs(d);
    entropy_enc_bin(e, ctx + kMotionCtxNz + comp, a != 0u);
    if (!a) return;
    entropy_enc_bin(e, ctx + kMotionCtxGt1 + comp, a > 1u);
    if (a > 1u) {                                                           // r = a - 2 as Exp-Golomb order 1: v = r + 2 = a
        const unsigned k = entropy_ilog2(a);
        for (unsigned i = 1; i < k; ++i) entropy_enc_bypass(e, 1u);
        entropy_enc_bypass(e, 0u);
        entropy_enc_bits(e, a, k);
    }
    entropy_enc_bypass(e, d < 0);
}

// false: malformed, a prefix of more than 14 ones
X266_HD inline bool entropy_motion_dec_diff(EntropyDec &d, uint16_t *ctx, unsigned comp, int *out)
{
    *out = 0;
    if (!entropy_dec_bin(d, ctx + kMotionCtxNz + comp)) return true;
    unsigned a = 1;
    if (entropy_dec_bin(d, ctx + kMotionCtxGt1 + comp)) {
        unsigned ones = 0;
        while (ones <= kMotionMaxPrefix && entropy_dec_bypass(d)) ++ones;
        if (ones > kMotionMaxPrefix) return false;
        const unsigned k = ones + 1u;                                       // 1 .. 15: a = 1 << k | suffix lies in 2 .. 65535
        a = (1u << k) | entropy_dec_bits(d, k);
    }
    *out = entropy_dec_bypass(d) ? -(int)a : (int)a;
    return true;
}

// the true difference of a partition's component from the pack stream's words: q and the low 16 bits w of d.  P = (int16_t)(q - (int16_t)w)
// is the predictor itself (the pack section's argument, read backwards), so d = q - P
X266_HD inline int entropy_motion_true_diff(uint16_t q_word, uint16_t w)
{
    const int q = (int16_t)q_word;
    const int p = (int16_t)(uint16_t)(q - (int16_t)w);
    return q - p;
}

// ---- a CTU ---------------------------------------------------------------------------------------------------------------------------------
// mask: well formed (motion_mask_well_formed); words: four per partition in coding order; ctx: the 7 contexts, initialised by the caller
X266_HD inline void entropy_motion_encode_ctu(EntropyEnc &e, const MotionCtu &g, uint64_t mask, const uint16_t *words, uint16_t *ctx)
{
    unsigned j = 0;
    for (uint64_t left = mask; left; left &= left - 1u, ++j) {              // at most 64 heads, ascending
        const unsigned h = (unsigned)__builtin_ctzll(left);
        const int k = motion_head_level(g, mask, h);
        for (int l = kPartLevels - 1; l > k; --l)
            if (motion_node_first(h, l) == h && motion_node_whole(g, h, l)) entropy_enc_bin(e, ctx + kMotionCtxSplit + (unsigned)l - 1u, 1u);
        if (k > 0) entropy_enc_bin(e, ctx + kMotionCtxSplit + (unsigned)k - 1u, 0u);
        const uint16_t *w = words + kMotionWordsPerPart * j;
        entropy_motion_enc_diff(e, ctx, 0u, entropy_motion_true_diff(w[0], w[2]));
        entropy_motion_enc_diff(e, ctx, 1u, entropy_motion_true_diff(w[1], w[3]));
    }
}

struct EntropyMotionCtu {
    uint64_t mask;
    uint32_t parts, bits, max_abs;
};

// The inverse: the mask it builds is well formed by construction.  words gets 0, 0, low16(dx), low16(dy) per partition and nothing beyond
// the payload.  false: malformed, and then *out and words hold a partial CTU that the caller replaces by the flat one.
X266_HD inline bool entropy_motion_decode_ctu(EntropyDec &d, const MotionCtu &g, uint16_t *ctx, uint16_t *words, EntropyMotionCtu *out)
{
    EntropyMotionCtu r = {0, 0, 0, 0};
    bool good = true;
    for (unsigned i = 0; i < 64u && good;) {
        if (!motion_block_exists(g, i)) {                                   // a node whose first block is outside the frame does not exist
            ++i;
            continue;
        }
        int k = 0;
        for (int l = kPartLevels - 1; l > 0; --l) {
            if (motion_node_first(i, l) != i || !motion_node_whole(g, i, l)) continue;      // begins elsewhere, or cut: no bin
            if (!entropy_dec_bin(d, ctx + kMotionCtxSplit + (unsigned)l - 1u)) {
                k = l;
                break;
            }
        }
        int dx = 0, dy = 0;
        good = entropy_motion_dec_diff(d, ctx, 0u, &dx) && entropy_motion_dec_diff(d, ctx, 1u, &dy);
        uint16_t *w = words + kMotionWordsPerPart * r.parts;
        w[0] = w[1] = 0;
        w[2] = (uint16_t)dx;
        w[3] = (uint16_t)dy;
        r.mask |= (uint64_t)1 << i;
        ++r.parts;
        r.bits += motion_part_bits(g, i, k, dx, dy);
        const uint32_t top = motion_abs(dx) > motion_abs(dy) ? motion_abs(dx) : motion_abs(dy);
        r.max_abs = top > r.max_abs ? top : r.max_abs;
        i += motion_node_blocks(k);
    }
    *out = r;
    return good;
}

// the flat CTU: what zero bytes decode to under every table (a zero bin is always the more probable half's side: code 0 < bound)
// ctx: room for the 7 contexts, overwritten
X266_HD inline void entropy_motion_flat_ctu(const MotionCtu &g, uint16_t *ctx, uint16_t *words, EntropyMotionCtu *out)
{
    for (unsigned i = 0; i < kEntropyMotionContexts; ++i) ctx[i] = kEntropyMotionDefault.p[i];
    EntropyDec d;
    entropy_dec_start(d, nullptr, 0u);
    entropy_motion_decode_ctu(d, g, ctx, words, out);
}

}  // namespace x266
