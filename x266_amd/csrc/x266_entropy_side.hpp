// x266_entropy_side.hpp -- the entropy coder of the side information: the one copy of the context layout, of the default table, of the
// canonical form, of the two mode lists and of a CTU's syntax that the kernels of entropy_side_kernels.hip (xEntropyEncodeSideGpu,
// xEntropyDecodeSideGpu), the host helpers xEntropySideDefaultInit, xEntropyEncodeSideCtu and xEntropyDecodeSideCtu and the host-only
// driver tests/cpp/entropy_side_rules_check.cpp share.  The statement is include/x266hip.h's ("the entropy coder of the side
// information"); the coder is x266_entropy.hpp's, used as it is.  Plain C++17.
//
// A CTU is held packed in five integers (EntropySideCtu), never in arrays: the kernels keep one CTU per lane in registers, and a private
// array indexed at run time would go to scratch.  The contexts are reached as ctx[i * stride]: the stride is 1 on the host; the kernels
// keep them in LDS context-major with the lane as the fast index.
// Every loop is bounded by the syntax: 6 regions, 5 list entries, 35 modes, 3 + 4 unary bins, 6 prefix ones, 5 suffix bits.
#pragma once

#include <cstdint>

#include "x266_entropy.hpp"

namespace x266 {

constexpr unsigned kEntropySideContexts = X266_ENTROPY_SIDE_CONTEXTS;
constexpr unsigned kEntropySideMaxBytes = X266_ENTROPY_SIDE_MAX_BYTES;
constexpr unsigned kSideRegions = 6, kSideModes = 35, kSideInter = 255, kSideQpMax = 51;
static_assert(kEntropySideContexts == 16, "kind 2, mpm, listed, coded 2, small 2, size 2, type 3, nz 2, gt1");

// kind, coded, small and nz take the component, 0 = luma; size and type take the bin of their truncated unary code
constexpr unsigned kSideCtxKind = 0, kSideCtxMpm = 2, kSideCtxListed = 3, kSideCtxCoded = 4, kSideCtxSmall = 6, kSideCtxSize = 8, kSideCtxType = 10, kSideCtxNz = 13,
                   kSideCtxGt1 = 15;
constexpr unsigned kSideMaxPrefix = 5;                                      // ones of the Exp-Golomb prefix: v = r + 1 <= 50

struct EntropySideInit {
    uint16_t p[kEntropySideContexts];
};
// nothing measured justifies a skew
constexpr EntropySideInit kEntropySideDefault = {{1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024}};

// the canonical CTU: region q's mode and qp are byte q, its class nibble q, its kind and its coded flag bit q
struct EntropySideCtu {
    uint64_t mode, qp;
    uint32_t cls, kind, coded;
};
X266_HD inline unsigned side_byte(uint64_t v, unsigned q) { return (unsigned)(v >> (8u * q)) & 0xFFu; }
X266_HD inline uint64_t side_with_byte(uint64_t v, unsigned q, unsigned b) { return (v & ~((uint64_t)0xFF << (8u * q))) | (uint64_t)b << (8u * q); }
X266_HD inline unsigned side_nibble(uint32_t v, unsigned q) { return (v >> (4u * q)) & 15u; }
X266_HD inline int side_clamp_qp(int q) { return q < 0 ? 0 : q > (int)kSideQpMax ? (int)kSideQpMax : q; }

// the class a transform runs for the byte c: the low four bits, a size-32 class of any type read as 3
X266_HD inline unsigned side_class(unsigned c)
{
    const unsigned k = c & 15u;
    return (k & 3u) == 3u ? 3u : k;
}

// the flat CTU: all inter, nothing coded; what zero bytes decode to under every table
X266_HD inline EntropySideCtu entropy_side_flat_ctu(int qp, int chroma_qp_offset)
{
    const uint64_t l = (uint64_t)qp, c = (uint64_t)side_clamp_qp(qp + chroma_qp_offset);
    EntropySideCtu s;
    s.mode = 0xFFFFFFFFFFFFull;
    s.qp = l | l << 8 | l << 16 | l << 24 | c << 32 | c << 40;
    s.cls = 0x333333u;
    s.kind = s.coded = 0;
    return s;
}

// an uncoded region's class and qp replaced by 3 and by the region's predictor: the form decode returns
X266_HD inline EntropySideCtu entropy_side_settle(EntropySideCtu s, int qp, int chroma_qp_offset)
{
    unsigned cur = (unsigned)qp;
    for (unsigned q = 0; q < kSideRegions; ++q) {
        const unsigned pred = q < 4u ? cur : q == 4u ? (unsigned)side_clamp_qp((int)cur + chroma_qp_offset) : side_byte(s.qp, 4u);
        if (!((s.coded >> q) & 1u)) {
            s.qp = side_with_byte(s.qp, q, pred);
            s.cls = (s.cls & ~(15u << (4u * q))) | 3u << (4u * q);
        }
        if (q < 4u) cur = side_byte(s.qp, q);
    }
    return s;
}

// The canonical form of a CTU's six entries of each array; a NULL array has the meaning the header gives it on encode.  kind must not be
// given without mode (the argument rules refuse it).
X266_HD inline EntropySideCtu entropy_side_canon(const uint8_t *kind, const uint8_t *mode, const uint8_t *cls, const uint8_t *qp_in, const uint32_t *nnz, int qp,
                                                 int chroma_qp_offset)
{
    EntropySideCtu s = entropy_side_flat_ctu(qp, chroma_qp_offset);
    for (unsigned q = 0; q < kSideRegions; ++q) {
        const unsigned from = q < 5u ? q : 4u;                              // one chroma kind and one chroma mode: entry 4's
        if (kind && kind[from]) {
            s.kind |= 1u << q;
            s.mode = side_with_byte(s.mode, q, mode[from] < 34u ? mode[from] : 34u);
        }
        if (!nnz || nnz[q]) s.coded |= 1u << q;
        if (cls) s.cls = (s.cls & ~(15u << (4u * q))) | side_class(cls[q]) << (4u * q);
        if (qp_in) s.qp = side_with_byte(s.qp, q, qp_in[q] < kSideQpMax ? qp_in[q] : kSideQpMax);
    }
    return entropy_side_settle(s, qp, chroma_qp_offset);
}

// ---- the mode lists ----------------------------------------------------------------------------------------------------------------------
// HEVC's three most probable modes of luma region q, entry i in byte i: A the left neighbour inside the CTU, B the one above
X266_HD inline uint32_t entropy_side_mpm(const EntropySideCtu &s, unsigned q)
{
    const unsigned A = (q & 1u) && ((s.kind >> (q - 1u)) & 1u) ? side_byte(s.mode, q - 1u) : 1u;
    const unsigned B = q >= 2u && ((s.kind >> (q - 2u)) & 1u) ? side_byte(s.mode, q - 2u) : 1u;
    if (A == B) {
        if (A < 2u) return 0u | 1u << 8 | 26u << 16;
        return A | (2u + ((A + 29u) & 31u)) << 8 | (2u + ((A - 1u) & 31u)) << 16;
    }
    const unsigned third = (A != 0u && B != 0u) ? 0u : (A != 1u && B != 1u) ? 1u : 26u;
    return A | B << 8 | third << 16;
}

// the chroma list, entry i in byte i, and its length in *len: the luma mode of region 0 if that is intra, then 0, 26, 10, 1, duplicates dropped
X266_HD inline uint64_t entropy_side_chroma_list(const EntropySideCtu &s, unsigned *len)
{
    uint64_t list = 0, seen = 0;
    unsigned n = 0;
    for (unsigned i = 0; i < 5u; ++i) {
        if (i == 0u && !(s.kind & 1u)) continue;
        const unsigned m = i == 0u ? side_byte(s.mode, 0u) : (0x010A1A00u >> (8u * (i - 1u))) & 0xFFu;
        if ((seen >> m) & 1u) continue;
        seen |= (uint64_t)1 << m;
        list |= (uint64_t)m << (8u * n);
        ++n;
    }
    *len = n;
    return list;
}

// the set of the first n entries of a list, bit m = mode m
X266_HD inline uint64_t side_list_set(uint64_t list, unsigned n)
{
    uint64_t set = 0;
    for (unsigned i = 0; i < n; ++i) set |= (uint64_t)1 << side_byte(list, i);
    return set;
}
// the index of mode m in the list, n if absent
X266_HD inline unsigned side_list_find(uint64_t list, unsigned n, unsigned m)
{
    unsigned at = n;
    for (unsigned i = n; i-- > 0;)
        if (side_byte(list, i) == m) at = i;
    return at;
}
// the rank of mode m among the modes outside the set, ascending, and its inverse (kSideModes or more: no such mode)
X266_HD inline unsigned side_rank(uint64_t set, unsigned m) { return m - (unsigned)__builtin_popcountll(set & (((uint64_t)1 << m) - 1u)); }
X266_HD inline unsigned side_unrank(uint64_t set, unsigned rank)
{
    unsigned m = 0;
    for (; m < kSideModes; ++m) {
        if ((set >> m) & 1u) continue;
        if (rank == 0u) break;
        --rank;
    }
    return m;
}

// ---- the elements ------------------------------------------------------------------------------------------------------------------------
// v <= top as truncated unary: v ones, then a zero if v < top.  ctx == nullptr: bypass bins, otherwise bin i has context i
template <class Sink>
X266_HD inline void side_enc_unary(Sink &e, uint16_t *ctx, unsigned stride, unsigned v, unsigned top)
{
    for (unsigned i = 0; i < top; ++i) {
        const unsigned bit = i < v;
        if (ctx) entropy_enc_bin(e, ctx + i * stride, bit);
        else entropy_enc_bypass(e, bit);
        if (!bit) break;
    }
}
X266_HD inline unsigned side_dec_unary(EntropyDec &d, uint16_t *ctx, unsigned stride, unsigned top)
{
    unsigned v = 0;
    for (; v < top; ++v)
        if (!(ctx ? entropy_dec_bin(d, ctx + v * stride) : entropy_dec_bypass(d))) break;
    return v;
}

// a mode against a list of n entries: the flag, then the index (truncated unary, bypass) or the rank among the other modes (5 bypass bits)
template <class Sink>
X266_HD inline void side_enc_mode(Sink &e, uint16_t *flag, uint64_t list, unsigned n, unsigned m)
{
    const unsigned at = side_list_find(list, n, m);
    entropy_enc_bin(e, flag, at < n);
    if (at < n) side_enc_unary(e, nullptr, 0u, at, n - 1u);
    else entropy_enc_bits(e, side_rank(side_list_set(list, n), m), 5u);
}
// kSideModes or more: malformed, a rank beyond the modes outside the list
X266_HD inline unsigned side_dec_mode(EntropyDec &d, uint16_t *flag, uint64_t list, unsigned n)
{
    if (entropy_dec_bin(d, flag)) return side_byte(list, side_dec_unary(d, nullptr, 0u, n - 1u));
    return side_unrank(side_list_set(list, n), entropy_dec_bits(d, 5u));
}

template <class Sink>
X266_HD inline void side_enc_class(Sink &e, uint16_t *ctx, unsigned stride, unsigned chroma, unsigned c)
{
    entropy_enc_bin(e, ctx + (kSideCtxSmall + chroma) * stride, c != 3u);
    if (c == 3u) return;
    side_enc_unary(e, ctx + kSideCtxSize * stride, stride, 2u - (c & 3u), 2u);
    side_enc_unary(e, ctx + kSideCtxType * stride, stride, c >> 2, 3u);
}
X266_HD inline unsigned side_dec_class(EntropyDec &d, uint16_t *ctx, unsigned stride, unsigned chroma)
{
    if (!entropy_dec_bin(d, ctx + (kSideCtxSmall + chroma) * stride)) return 3u;
    const unsigned size = 2u - side_dec_unary(d, ctx + kSideCtxSize * stride, stride, 2u);
    return size | side_dec_unary(d, ctx + kSideCtxType * stride, stride, 3u) << 2;
}

// the qp difference dq, |dq| <= 51
template <class Sink>
X266_HD inline void side_enc_dqp(Sink &e, uint16_t *ctx, unsigned stride, unsigned chroma, int dq)
{
    const unsigned a = (unsigned)(dq < 0 ? -dq : dq);
    entropy_enc_bin(e, ctx + (kSideCtxNz + chroma) * stride, a != 0u);
    if (!a) return;
    entropy_enc_bin(e, ctx + kSideCtxGt1 * stride, a > 1u);
    if (a > 1u) {                                                           // r = a - 2 as Exp-Golomb order 0: v = r + 1
        const unsigned v = a - 1u, k = entropy_ilog2(v);
        for (unsigned i = 0; i < k; ++i) entropy_enc_bypass(e, 1u);
        entropy_enc_bypass(e, 0u);
        entropy_enc_bits(e, v, k);
    }
    entropy_enc_bypass(e, dq < 0);
}
// false: malformed, a prefix of more than 5 ones
X266_HD inline bool side_dec_dqp(EntropyDec &d, uint16_t *ctx, unsigned stride, unsigned chroma, int *dq)
{
    *dq = 0;
    if (!entropy_dec_bin(d, ctx + (kSideCtxNz + chroma) * stride)) return true;
    unsigned a = 1;
    if (entropy_dec_bin(d, ctx + kSideCtxGt1 * stride)) {
        unsigned k = 0;
        for (; k <= kSideMaxPrefix; ++k)
            if (!entropy_dec_bypass(d)) break;
        if (k > kSideMaxPrefix) return false;
        a = ((1u << k) | entropy_dec_bits(d, k)) + 1u;                      // at most 64: held against 0 .. 51 by the caller
    }
    *dq = entropy_dec_bypass(d) ? -(int)a : (int)a;
    return true;
}

// ---- a CTU -------------------------------------------------------------------------------------------------------------------------------
// s: canonical (entropy_side_canon or a decoder's output); ctx: the 16 contexts at ctx[i * stride], initialised by the caller
template <class Sink>
X266_HD inline void entropy_side_encode_ctu(Sink &e, const EntropySideCtu &s, uint16_t *ctx, unsigned stride, int qp, int chroma_qp_offset)
{
    unsigned cur = (unsigned)qp, u = 0;
    for (unsigned q = 0; q < kSideRegions; ++q) {
        const unsigned chroma = q >= 4u, intra = (s.kind >> q) & 1u;
        if (q < 5u) {                                                       // V has U's kind and mode
            entropy_enc_bin(e, ctx + (kSideCtxKind + chroma) * stride, intra);
            if (intra && !chroma) side_enc_mode(e, ctx + kSideCtxMpm * stride, entropy_side_mpm(s, q), 3u, side_byte(s.mode, q));
            if (intra && chroma) {
                unsigned n = 0;
                const uint64_t list = entropy_side_chroma_list(s, &n);
                side_enc_mode(e, ctx + kSideCtxListed * stride, list, n, side_byte(s.mode, q));
            }
        }
        const unsigned pred = q < 4u ? cur : q == 4u ? (unsigned)side_clamp_qp((int)cur + chroma_qp_offset) : u;
        const unsigned coded = (s.coded >> q) & 1u, own = coded ? side_byte(s.qp, q) : pred;
        entropy_enc_bin(e, ctx + (kSideCtxCoded + chroma) * stride, coded);
        if (coded) {
            side_enc_class(e, ctx, stride, chroma, side_nibble(s.cls, q));
            side_enc_dqp(e, ctx, stride, chroma, (int)own - (int)pred);
        }
        if (q < 4u) cur = own;
        if (q == 4u) u = own;
    }
}

// The inverse; the result is canonical.  false: malformed, and then *out is not written (the caller takes the flat CTU).
X266_HD inline bool entropy_side_decode_ctu(EntropyDec &d, uint16_t *ctx, unsigned stride, int qp, int chroma_qp_offset, EntropySideCtu *out)
{
    EntropySideCtu s = entropy_side_flat_ctu(qp, chroma_qp_offset);
    unsigned cur = (unsigned)qp, u = 0;
    for (unsigned q = 0; q < kSideRegions; ++q) {
        const unsigned chroma = q >= 4u;
        if (q < 5u) {
            if (entropy_dec_bin(d, ctx + (kSideCtxKind + chroma) * stride)) {
                unsigned n = 3, m;
                if (!chroma) {
                    m = side_dec_mode(d, ctx + kSideCtxMpm * stride, entropy_side_mpm(s, q), 3u);
                } else {
                    const uint64_t list = entropy_side_chroma_list(s, &n);
                    m = side_dec_mode(d, ctx + kSideCtxListed * stride, list, n);
                }
                if (m >= kSideModes) return false;
                s.kind |= 1u << q;
                s.mode = side_with_byte(s.mode, q, m);
            }
        } else if ((s.kind >> 4) & 1u) {
            s.kind |= 1u << 5;
            s.mode = side_with_byte(s.mode, 5u, side_byte(s.mode, 4u));
        }
        const unsigned pred = q < 4u ? cur : q == 4u ? (unsigned)side_clamp_qp((int)cur + chroma_qp_offset) : u;
        unsigned own = pred;
        if (entropy_dec_bin(d, ctx + (kSideCtxCoded + chroma) * stride)) {
            s.coded |= 1u << q;
            s.cls = (s.cls & ~(15u << (4u * q))) | side_dec_class(d, ctx, stride, chroma) << (4u * q);
            int dq = 0;
            if (!side_dec_dqp(d, ctx, stride, chroma, &dq)) return false;
            const int v = (int)pred + dq;
            if (v < 0 || v > (int)kSideQpMax) return false;
            own = (unsigned)v;
        }
        s.qp = side_with_byte(s.qp, q, own);
        if (q < 4u) cur = own;
        if (q == 4u) u = own;
    }
    *out = s;
    return true;
}

// the six entries of each output array from a canonical CTU; a NULL array is not written
X266_HD inline void entropy_side_store(const EntropySideCtu &s, uint8_t *kind, uint8_t *mode, uint8_t *cls, uint8_t *qp_out, uint32_t *nnz)
{
    for (unsigned q = 0; q < kSideRegions; ++q) {
        if (kind) kind[q] = (uint8_t)((s.kind >> q) & 1u);
        if (mode) mode[q] = (uint8_t)side_byte(s.mode, q);
        if (cls) cls[q] = (uint8_t)side_nibble(s.cls, q);
        if (qp_out) qp_out[q] = (uint8_t)side_byte(s.qp, q);
        if (nnz) nnz[q] = (s.coded >> q) & 1u;
    }
}

}  // namespace x266
