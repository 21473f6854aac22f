// x266_aq.hpp -- source analysis: the one copy of the arithmetic behind xAqStatsGpu, xAqDecideGpu (aq_kernels.hip) and the host call
// xWeightsFromTotals.  The statement is include/x266hip.h's ("source analysis"); tests/_aq_ref.py restates it in numpy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace x266 {

constexpr unsigned kAqTotalsThreads = 1024;        // lanes of the totals' one workgroup
constexpr unsigned kAqTotalsChunk = 2048;          // records it takes per full step (xAqTotalsChunk): four 16-byte halves per lane
constexpr int kAqFixedRefQ8 = 3693;                // mode 1: 256 * 14.427
constexpr int kAqOffsetMaxQ8 = 3072;               // a tile's offset is held to +-12 qp steps

// floor(256 * log2(max(e, 1))): the integer part from the leading bit, eight fraction bits by squaring the mantissa
__host__ __device__ inline uint32_t aq_log2_q8(uint32_t e)
{
    if (e == 0) e = 1;
    const unsigned k = 31u - (unsigned)__builtin_clz(e);
    uint64_t m = (uint64_t)e << (31u - k);                                  // the mantissa in [2^31, 2^32)
    uint32_t f = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m = (m * m) >> 31;                                                  // in [2^31, 2^33)
        f <<= 1;
        if (m >> 32) {
            f |= 1u;
            m >>= 1;
        }
    }
    return (k << 8) | f;
}

// the three planes' sums of squared deviations (each times its sample count): every product unsigned -- sum_y^2 passes 2^31
__host__ __device__ inline uint32_t aq_energy(uint32_t sum_y, uint32_t ssq_y, uint32_t sum_u, uint32_t ssq_u, uint32_t sum_v, uint32_t ssq_v)
{
    return (ssq_y - ((sum_y * sum_y) >> 8)) + (ssq_u - ((sum_u * sum_u) >> 6)) + (ssq_v - ((sum_v * sum_v) >> 6));
}

// the reference a tile's log2 is held against; sum_log2 = d_total[6]
__host__ __device__ inline int aq_ref_q8(int mode, int64_t sum_log2, int64_t n_tiles)
{
    return mode == 1 ? kAqFixedRefQ8 : (int)((sum_log2 + n_tiles / 2) / n_tiles);
}

// a tile's qp offset in Q8
__host__ __device__ inline int aq_offset_q8(int strength_q8, int log2_q8, int ref_q8)
{
    const int off = (strength_q8 * (log2_q8 - ref_q8)) >> 8;                // arithmetic shift; |product| < 2^23
    return off < -kAqOffsetMaxQ8 ? -kAqOffsetMaxQ8 : off > kAqOffsetMaxQ8 ? kAqOffsetMaxQ8 : off;
}

// the mean of n offsets (their sum s) rounded to whole qp steps: floor((2 s + 256 n) / (512 n)); no tile, no change
__host__ __device__ inline int aq_delta(int s, int n)
{
    if (n <= 0) return 0;
    const int num = 2 * s + 256 * n, den = 512 * n;
    const int q = num / den;
    return num % den < 0 ? q - 1 : q;
}

// the byte of region q of a CTU
__host__ __device__ inline unsigned aq_region_qp(int base_qp, int delta, int q, int chroma_qp_offset)
{
    const int qp = base_qp + delta + (q >= 4 ? chroma_qp_offset : 0);
    return (unsigned)(qp < 0 ? 0 : qp > 51 ? 51 : qp);
}

#ifdef __HIPCC__
// The six qp bytes of a CTU from its tiles' offsets (xAqDecideGpu, xLaTreeQpGpu): a row of 16 lanes per CTU, lane i = lane & 15 its tile
// (i & 3, i >> 2) with offset s and n = 1, or s = n = 0 for a tile outside the frame.  Every lane of the wave calls it.
__device__ __forceinline__ void aq_ctu_qp(int s, int n, unsigned lane, bool ctu_ok, size_t ctu, int base_qp, int chroma_qp_offset, uint8_t *qp)
{
    const unsigned i = lane & 15;
    // quadrant q = ((i >> 3) & 1) * 2 + ((i >> 1) & 1): its four tiles differ in bits 0 and 2 of i; the CTU's in all four bits
    int packed = s * 32 + n;                                                // |s| <= 16 * 3072 and n <= 16 over a CTU: one register, s = packed >> 5 after
    packed += __shfl_xor(packed, 1, 64);                                    // the sums (n < 32, and the shift is arithmetic)
    packed += __shfl_xor(packed, 4, 64);
    int all = packed + __shfl_xor(packed, 2, 64);
    all += __shfl_xor(all, 8, 64);
    // lanes 0..3 of the row take quadrant i from its first lane, lanes 4 and 5 the whole CTU
    const int from = (int)(lane & 48u) + (int)((i & 1) * 2 + ((i >> 1) & 1) * 8);
    const int quad = __shfl(packed, from, 64);
    if (ctu_ok && i < 6 && qp) {
        const int v = i < 4 ? quad : all;
        const int count = v & 31, sum = (v - count) / 32;
        qp[ctu * 6 + i] = (uint8_t)aq_region_qp(base_qp, aq_delta(sum, count), (int)i, chroma_qp_offset);
    }
}
#endif

// ---- fade weights from two frames' totals (host only: the variance products pass 2^63 at 8K) -----------------------------------------------
typedef unsigned __int128 aq_u128;
typedef __int128 aq_i128;

inline uint64_t aq_isqrt(aq_u128 x)                                         // floor(sqrt(x)) for x < 2^126
{
    aq_u128 r = 0, bit = (aq_u128)1 << 124;
    while (bit > x) bit >>= 2;
    for (; bit; bit >>= 2) {
        if (x >= r + bit) {
            x -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return (uint64_t)r;
}

// plane 0 = Y, 1 = U, 2 = V of totals {sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v, .., n_tiles}; d = log2_denom of the plane
inline void aq_plane_weight(const int64_t cur[8], const int64_t ref[8], int plane, unsigned d, int16_t *w_out, int16_t *o_out)
{
    const aq_u128 n = (aq_u128)(uint64_t)cur[7] * (plane ? 64u : 256u);
    const aq_u128 sum_cur = (uint64_t)cur[2 * plane], ssq_cur = (uint64_t)cur[2 * plane + 1];
    const aq_u128 sum_ref = (uint64_t)ref[2 * plane], ssq_ref = (uint64_t)ref[2 * plane + 1];
    const aq_u128 var_cur = ssq_cur * n - sum_cur * sum_cur, var_ref = ssq_ref * n - sum_ref * sum_ref;
    int64_t w = (int64_t)1 << d;
    if (var_ref != 0) w = (int64_t)((aq_isqrt((var_cur << (2 * d + 2)) / var_ref) + 1) >> 1);
    w = w < 1 ? 1 : w > 127 ? 127 : w;
    const aq_i128 scale = (aq_i128)1 << d;
    const aq_i128 num = 2 * ((aq_i128)sum_cur * scale - (aq_i128)sum_ref * w) + (aq_i128)n * scale, den = 2 * (aq_i128)n * scale;
    aq_i128 o = num / den;
    if (num % den < 0) --o;
    *w_out = (int16_t)w;
    *o_out = (int16_t)(o < -128 ? -128 : o > 127 ? 127 : o);
}

}  // namespace x266
