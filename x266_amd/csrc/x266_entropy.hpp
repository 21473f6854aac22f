// x266_entropy.hpp -- the entropy coder of the level stream: the one copy of the context layout, of the default table, of the range
// coder and of a region's syntax that the kernels of entropy_kernels.hip and the host helpers xEntropyEncodeRegion, xEntropyDecodeRegion
// and xEntropyDefaultInit share.  The statement is include/x266hip.h's (xEntropyEncodeLevelsGpu ...); the scan and the CG origins are
// x266_levels.hpp's; g of pos() and rem() are restated here from x266_rdoq.hpp so that this file stays plain C++ for the host-only
// driver (tests/cpp/entropy_rules_check.cpp); tests/test_entropy_ref.py holds the bin counts against xLastPosBits and xLevelBits.
// The syntax walks are templates over their sink: EntropyEnc codes, EntropyCounter (below) counts the bins per context for the
// statistics (xEntropyCountRegion, xEntropyStatsSideGpu ...); the table rule of xEntropyInitFromCounts is here as well.
//
// What the kernels rely on:
//   * a probability that starts in 31 .. 2017 stays there: p += (2048 - p) >> 5 stops at 2017, p -= p >> 5 at 31.  With range >= 2^24
//     before a bin, bound = (range >> 11) * p lies in [2^13 * 31, range - 2^13 * 31]: both halves are above 2^16, ONE byte shift brings
//     the range back to 2^24 or more.  A bypass bin halves a range of at least 2^24: one shift as well.  No renormalisation loop.
//   * every loop here has a trip count bounded by the syntax (blocks, CGs, 16 positions, 2n - 1 prefix bins, 15 Exp-Golomb prefix bins,
//     14 suffix bits) or by the bytes put out so far (the pending run of 0xFF): a decoder fed garbage terminates.
//   * the sink counts every byte and stores only those below its capacity: no bound on the substream is needed for memory safety.
#pragma once

#include <cstdint>

#include "x266_levels.hpp"

namespace x266 {

constexpr unsigned kEntropyCtxPerSize = 25;
constexpr unsigned kEntropyContexts = 4 * kEntropyCtxPerSize;
constexpr unsigned kEntropyProbMin = 31, kEntropyProbMax = 2017;
constexpr unsigned kEntropyMaxBytes = X266_ENTROPY_MAX_BYTES;
static_assert(kEntropyContexts == X266_ENTROPY_CONTEXTS, "the header's count");
static_assert(kEntropyMaxBytes % 16 == 0, "the staging slabs hold whole 16-byte chunks");

// the contexts of one block size, in the order of the table: cbf, last x (bin 0..8), last y (bin 0..8), cgf, sig (class 0..2), gt1, gt2
constexpr unsigned kCtxCbf = 0, kCtxLastX = 1, kCtxLastY = 10, kCtxCgf = 19, kCtxSig = 20, kCtxGt1 = 23, kCtxGt2 = 24;

struct EntropyInit {
    uint16_t p[kEntropyContexts];
};
// p0 = 2048 * 2^(-c0/16) / (2^(-c0/16) + 2^(-c1/16)) of the costs of x266_rdoq.hpp, rounded; 1024 for cbf and the last-position prefix
#define X266_ENTROPY_ROW 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1385, 723, 1242, 1609, 1325, 1263
constexpr EntropyInit kEntropyDefault = {{X266_ENTROPY_ROW, X266_ENTROPY_ROW, X266_ENTROPY_ROW, X266_ENTROPY_ROW}};
#undef X266_ENTROPY_ROW

// scan position of CG (cgx, cgy) in a block of N = 4 << k, and of (x, y) in a 4x4 CG: the inverses of x266_levels.hpp's tables
struct EntropyTab {
    uint8_t cg[4][64], pos4[16];
};
constexpr EntropyTab make_entropy_tab()
{
    EntropyTab t = {};
    for (unsigned k = 0; k < 4; ++k) {
        const unsigned m = 1u << k;
        const LevelDiag d = level_diag(m);
        for (unsigned s = 0; s < m * m; ++s) t.cg[k][d.y[s] * m + d.x[s]] = (uint8_t)s;
    }
    const LevelDiag d4 = level_diag(4);
    for (unsigned i = 0; i < 16; ++i) t.pos4[d4.y[i] * 4 + d4.x[i]] = (uint8_t)i;
    return t;
}
X266_HD inline unsigned entropy_cg_scan(unsigned k, unsigned cgx, unsigned cgy)
{
    constexpr EntropyTab t = make_entropy_tab();
    return t.cg[k & 3u][((cgy << k) + cgx) & 63u];
}
X266_HD inline unsigned entropy_pos4(unsigned x, unsigned y)
{
    constexpr EntropyTab t = make_entropy_tab();
    return t.pos4[(y * 4u + x) & 15u];
}

// floor(log2 t), t >= 1
X266_HD inline unsigned entropy_ilog2(unsigned t) { return 31u - (unsigned)__builtin_clz(t); }

// the group index g of one coordinate of the last position, as rdoq_last_pos forms it
X266_HD inline unsigned entropy_last_group(unsigned t)
{
    if (t < 4u) return t;
    const unsigned k = entropy_ilog2(t);
    return 2u * k + ((t >> (k - 1u)) & 1u);
}

// ---- the encoder -----------------------------------------------------------------------------------------------------------------------
struct EntropyEnc {
    uint64_t low;
    uint32_t range, pending;        // pending: the cache byte and the 0xFF bytes behind it that still wait for a carry
    uint32_t cap, n, last;          // bytes the sink holds; bytes put so far (the leading one not counted); index + 1 of the last non-zero one
    uint32_t ctx_bins, bypass_bins;
    uint8_t *buf;
    uint8_t cache;
    bool lead;                      // the leading byte, always 0, has not been dropped yet
};

X266_HD inline void entropy_enc_start(EntropyEnc &e, uint8_t *buf, uint32_t cap)
{
    e.low = 0;
    e.range = 0xFFFFFFFFu;
    e.pending = 1;
    e.cap = buf ? cap : 0u;
    e.n = e.last = e.ctx_bins = e.bypass_bins = 0;
    e.buf = buf;
    e.cache = 0;
    e.lead = true;
}

X266_HD inline void entropy_put(EntropyEnc &e, uint8_t b)
{
    if (e.lead) {
        e.lead = false;
        return;
    }
    if (e.n < e.cap) e.buf[e.n] = b;
    ++e.n;
    if (b) e.last = e.n;
}

X266_HD inline void entropy_shift_low(EntropyEnc &e)
{
    if ((uint32_t)e.low < 0xFF000000u || (e.low >> 32) != 0) {
        const uint8_t carry = (uint8_t)(e.low >> 32);
        for (; e.pending; --e.pending) {                                     // at most the bytes put out so far + 1
            entropy_put(e, (uint8_t)(e.cache + carry));
            e.cache = 0xFF;
        }
        e.cache = (uint8_t)(e.low >> 24);
    }
    ++e.pending;
    e.low = (e.low & 0x00FFFFFFull) << 8;
}

X266_HD inline void entropy_enc_bin(EntropyEnc &e, uint16_t *ctx, unsigned bit)
{
    const uint32_t p = *ctx, bound = (e.range >> 11) * p;
    if (bit) {
        e.low += bound;
        e.range -= bound;
        *ctx = (uint16_t)(p - (p >> 5));
    } else {
        e.range = bound;
        *ctx = (uint16_t)(p + ((2048u - p) >> 5));
    }
    if (e.range < (1u << 24)) {
        e.range <<= 8;
        entropy_shift_low(e);
    }
    ++e.ctx_bins;
}

X266_HD inline void entropy_enc_bypass(EntropyEnc &e, unsigned bit)
{
    e.range >>= 1;
    if (bit) e.low += e.range;
    if (e.range < (1u << 24)) {
        e.range <<= 8;
        entropy_shift_low(e);
    }
    ++e.bypass_bins;
}

// ---- the counting sink ---------------------------------------------------------------------------------------------------------------------
// What the syntax walks below (entropy_enc_last, entropy_enc_level, entropy_encode_region and the side syntax of x266_entropy_side.hpp) take
// in place of an EntropyEnc to COUNT the context bins instead of coding them: the walks are templates over their sink, so that the
// statistics (xEntropyCountRegion, xEntropyCountSideCtu, xEntropyStatsSideGpu) run the one copy of each syntax.  `base` is the address
// the walk's context 0 has (never read or written through; the side walk is told a stride of 1); context c's zero bins are counted in
// counts[2 c * PITCH], its one bins in counts[(2 c + 1) * PITCH].  Bypass bins are not counted.
template <class T, unsigned PITCH>
struct EntropyCounter {
    T *counts;
    const uint16_t *base;
};
template <class T, unsigned PITCH>
X266_HD inline void entropy_enc_bin(EntropyCounter<T, PITCH> &e, uint16_t *ctx, unsigned bit)
{
    const unsigned c = (unsigned)(ctx - e.base);
    e.counts[(2u * c + (bit ? 1u : 0u)) * PITCH] += 1;
}
template <class T, unsigned PITCH>
X266_HD inline void entropy_enc_bypass(EntropyCounter<T, PITCH> &, unsigned)
{
}

// the initial probability of a context that took z zero and o one bins, both below 2^51: 2048 z / (z + o) rounded half up, held to the
// interval the adaptation never leaves (xEntropyInitFromCounts)
inline uint16_t entropy_init_from_counts(uint64_t z, uint64_t o)
{
    const uint64_t n = z + o;
    if (n == 0) return 1024;
    const uint64_t p = (4096u * z + n) / (2u * n);
    return (uint16_t)(p < kEntropyProbMin ? kEntropyProbMin : p > kEntropyProbMax ? kEntropyProbMax : p);
}

// the `count` low bits of value, most significant first; any count up to 32 (the level syntax asks for 14 at most, the motion syntax 15)
template <class Sink>
X266_HD inline void entropy_enc_bits(Sink &e, unsigned value, unsigned count)
{
    for (unsigned i = count; i-- > 0;) entropy_enc_bypass(e, (value >> i) & 1u);
}

// n_bytes of the substream: the leading byte and the trailing zero bytes are not part of it
X266_HD inline uint32_t entropy_enc_finish(EntropyEnc &e)
{
    e.low = (e.low + 0xFFFFFFull) & ~0xFFFFFFull;
    for (int i = 0; i < 5; ++i) entropy_shift_low(e);
    return e.last;
}

// one coordinate t of the last position of a block of 1 << n: ctx points at the coordinate's nine prefix contexts
template <class Sink>
X266_HD inline void entropy_enc_last(Sink &e, uint16_t *ctx, unsigned t, unsigned n)
{
    const unsigned g = entropy_last_group(t), top = 2u * n - 1u;
    for (unsigned i = 0; i < g; ++i) entropy_enc_bin(e, ctx + i, 1u);
    if (g < top) entropy_enc_bin(e, ctx + g, 0u);
    if (g >= 4u) entropy_enc_bits(e, t, (g >> 1) - 1u);                     // the bits of t below the two that g holds
}

// a non-zero level l at a position whose significance is already coded
template <class Sink>
X266_HD inline void entropy_enc_level(Sink &e, uint16_t *ctx, int l)
{
    const unsigned a = (unsigned)(l < 0 ? -l : l);
    entropy_enc_bin(e, ctx + kCtxGt1, a > 1u);
    if (a > 1u) {
        entropy_enc_bin(e, ctx + kCtxGt2, a > 2u);
        if (a > 2u) {
            const unsigned r = a - 3u;
            for (unsigned i = 0; i < (r < 3u ? r : 3u); ++i) entropy_enc_bypass(e, 1u);
            if (r < 3u) {
                entropy_enc_bypass(e, 0u);
            } else {
                const unsigned v = r - 2u, k = entropy_ilog2(v);               // Exp-Golomb order 0 of r - 3: v = r - 3 + 1
                for (unsigned i = 0; i < k; ++i) entropy_enc_bypass(e, 1u);
                entropy_enc_bypass(e, 0u);
                entropy_enc_bits(e, v, k);
            }
        }
    }
    entropy_enc_bypass(e, l < 0);
}

// A region: `level` its 1024 levels in the region's own layout, k = class & 3, cg_mask bit g set when CG g has a non-zero level,
// ctx the 25 contexts of this block size, initialised by the caller.  Only coded CGs are read.
template <class Sink>
X266_HD inline void entropy_encode_region(Sink &e, const int16_t *level, unsigned k, uint64_t cg_mask, uint16_t *ctx)
{
    const unsigned n = k + 2u, size = 4u << k, per_block = 1u << (2u * k), blocks = 64u >> (2u * k);
    for (unsigned blk = 0; blk < blocks; ++blk) {
        const uint64_t cgs = (cg_mask >> (blk * per_block)) & (per_block == 64u ? ~0ull : (1ull << per_block) - 1ull);
        entropy_enc_bin(e, ctx + kCtxCbf, cgs != 0);
        if (!cgs) continue;
        const unsigned sp = 63u - (unsigned)__builtin_clzll(cgs);
        const int16_t *last_cg = level + level_cg_origin(k, blk * per_block + sp);
        unsigned ip = 0;                                                     // the last non-zero scan position of CG sp
        for (unsigned i = 0; i < 16; ++i) {
            const unsigned yx = level_scan4(i);
            if (last_cg[(yx >> 2) * size + (yx & 3u)] != 0) ip = i;
        }
        {
            const unsigned yx = level_scan4(ip), org = level_cg_origin(k, blk * per_block + sp) - blk * size * size;
            entropy_enc_last(e, ctx + kCtxLastX, org % size + (yx & 3u), n);
            entropy_enc_last(e, ctx + kCtxLastY, org / size + (yx >> 2), n);
        }
        for (unsigned s = 0; s <= sp; ++s) {
            const bool coded = (cgs >> s) & 1u;
            if (s > 0 && s < sp) entropy_enc_bin(e, ctx + kCtxCgf, coded);
            if (!coded && s > 0) continue;                                  // CG 0 and CG sp are implied coded
            const int16_t *cg = level + level_cg_origin(k, blk * per_block + s);
            const unsigned end = s == sp ? ip : 15u;
            for (unsigned i = 0; i <= end; ++i) {
                const unsigned yx = level_scan4(i);
                const int l = cg[(yx >> 2) * size + (yx & 3u)];
                if (!(s == sp && i == ip)) entropy_enc_bin(e, ctx + kCtxSig + (s ? 2u : i ? 1u : 0u), l != 0);
                if (l) entropy_enc_level(e, ctx, l);
            }
        }
    }
}

// ---- the decoder -----------------------------------------------------------------------------------------------------------------------
struct EntropyDec {
    const uint8_t *buf;
    uint32_t n_bytes, at;
    uint32_t range, code;
};

X266_HD inline uint32_t entropy_next_byte(EntropyDec &d)
{
    const uint32_t b = d.at < d.n_bytes ? d.buf[d.at] : 0u;                 // zeros beyond the end of the substream
    ++d.at;
    return b;
}

X266_HD inline void entropy_dec_start(EntropyDec &d, const uint8_t *buf, uint32_t n_bytes)
{
    d.buf = buf;
    d.n_bytes = buf ? n_bytes : 0u;
    d.at = 0;
    d.range = 0xFFFFFFFFu;
    d.code = 0;
    for (int i = 0; i < 4; ++i) d.code = (d.code << 8) | entropy_next_byte(d);
}

X266_HD inline unsigned entropy_dec_bin(EntropyDec &d, uint16_t *ctx)
{
    const uint32_t p = *ctx, bound = (d.range >> 11) * p;
    unsigned bit;
    if (d.code < bound) {
        d.range = bound;
        *ctx = (uint16_t)(p + ((2048u - p) >> 5));
        bit = 0;
    } else {
        d.code -= bound;
        d.range -= bound;
        *ctx = (uint16_t)(p - (p >> 5));
        bit = 1;
    }
    if (d.range < (1u << 24)) {
        d.range <<= 8;
        d.code = (d.code << 8) | entropy_next_byte(d);
    }
    return bit;
}

X266_HD inline unsigned entropy_dec_bypass(EntropyDec &d)
{
    d.range >>= 1;
    unsigned bit = 0;
    if (d.code >= d.range) {
        d.code -= d.range;
        bit = 1;
    }
    if (d.range < (1u << 24)) {
        d.range <<= 8;
        d.code = (d.code << 8) | entropy_next_byte(d);
    }
    return bit;
}

X266_HD inline unsigned entropy_dec_bits(EntropyDec &d, unsigned count)
{
    unsigned v = 0;
    for (unsigned i = 0; i < count; ++i) v = (v << 1) | entropy_dec_bypass(d);
    return v;
}

// g <= 2n - 1 gives t < 1 << n: for g >= 4, t = (2 + (g & 1)) << ((g >> 1) - 1) | suffix with (g >> 1) <= n - 1
X266_HD inline unsigned entropy_dec_last(EntropyDec &d, uint16_t *ctx, unsigned n)
{
    const unsigned top = 2u * n - 1u;
    unsigned g = 0;
    while (g < top && entropy_dec_bin(d, ctx + g)) ++g;
    if (g < 4u) return g;
    const unsigned low_bits = (g >> 1) - 1u;
    return ((2u + (g & 1u)) << low_bits) | entropy_dec_bits(d, low_bits);
}

// the level at a significant position; false: malformed
X266_HD inline bool entropy_dec_level(EntropyDec &d, uint16_t *ctx, int *l)
{
    unsigned a = 1;
    if (entropy_dec_bin(d, ctx + kCtxGt1)) {
        a = 2;
        if (entropy_dec_bin(d, ctx + kCtxGt2)) {
            unsigned r = 0;
            while (r < 3u && entropy_dec_bypass(d)) ++r;
            if (r == 3u) {
                unsigned k = 0;
                while (k < 15u && entropy_dec_bypass(d)) ++k;
                if (k > 14u) return false;
                r = 2u + ((1u << k) | entropy_dec_bits(d, k));              // r - 2 = v = 1 << k | suffix
            }
            a = 3u + r;
        }
    }
    const unsigned negative = entropy_dec_bypass(d);
    if (a > 32768u || (a == 32768u && !negative)) return false;
    *l = negative ? -(int)a : (int)a;
    return true;
}

// The inverse of entropy_encode_region.  `level` must hold 1024 zeros: only non-zero levels are written.  false: malformed, and then
// level holds a partial region that the caller clears.
X266_HD inline bool entropy_decode_region(EntropyDec &d, int16_t *level, unsigned k, uint16_t *ctx, uint32_t *n_nz)
{
    const unsigned n = k + 2u, size = 4u << k, per_block = 1u << (2u * k), blocks = 64u >> (2u * k);
    uint32_t count = 0;
    for (unsigned blk = 0; blk < blocks; ++blk) {
        if (!entropy_dec_bin(d, ctx + kCtxCbf)) continue;
        const unsigned u = entropy_dec_last(d, ctx + kCtxLastX, n), v = entropy_dec_last(d, ctx + kCtxLastY, n);
        const unsigned sp = entropy_cg_scan(k, u >> 2, v >> 2), ip = entropy_pos4(u & 3u, v & 3u);
        for (unsigned s = 0; s <= sp; ++s) {
            bool coded = true;
            if (s > 0 && s < sp) coded = entropy_dec_bin(d, ctx + kCtxCgf);
            if (!coded) continue;
            int16_t *cg = level + level_cg_origin(k, blk * per_block + s);
            const unsigned end = s == sp ? ip : 15u;
            for (unsigned i = 0; i <= end; ++i) {
                bool sig = true;
                if (!(s == sp && i == ip)) sig = entropy_dec_bin(d, ctx + kCtxSig + (s ? 2u : i ? 1u : 0u));
                if (!sig) continue;
                int l = 0;
                if (!entropy_dec_level(d, ctx, &l)) return false;
                const unsigned yx = level_scan4(i);
                cg[(yx >> 2) * size + (yx & 3u)] = (int16_t)l;
                ++count;
            }
        }
    }
    *n_nz = count;
    return true;
}

// cg_mask of a region on the host (the kernels form it by a ballot)
inline uint64_t entropy_cg_mask(const int16_t *level, unsigned k)
{
    const unsigned size = 4u << k;
    uint64_t mask = 0;
    for (unsigned g = 0; g < 64; ++g) {
        const int16_t *cg = level + level_cg_origin(k, g);
        bool any = false;
        for (unsigned y = 0; y < 4; ++y)
            for (unsigned x = 0; x < 4; ++x) any = any || cg[y * size + x] != 0;
        mask |= (uint64_t)any << g;
    }
    return mask;
}

#if defined(__HIPCC__)
typedef int entropy_v4i __attribute__((ext_vector_type(4)));
// The words [phase, phase + n_words) of src to the same places of dst; word 0 of both is 16-byte aligned (an LDS slab on one side, the
// stream at offset - phase on the other): whole 16-byte chunks, single words only at the two ragged ends a substream shares with its
// neighbours.  Nothing outside the substream's own words is read or written.
__device__ __forceinline__ void substream_copy(uint16_t *dst, const uint16_t *src, unsigned phase, unsigned n_words, unsigned lane)
{
    const unsigned n_chunks = (phase + n_words + 7u) >> 3;
    for (unsigned c = lane; c < n_chunks; c += 64) {
        const unsigned lo = c * 8;
        if (lo >= phase && lo + 8 <= phase + n_words) {
            *reinterpret_cast<entropy_v4i *>(dst + lo) = *reinterpret_cast<const entropy_v4i *>(src + lo);
        } else {
            for (unsigned w = lo; w < lo + 8; ++w)
                if (w >= phase && w < phase + n_words) dst[w] = src[w];
        }
    }
}
#endif

}  // namespace x266
