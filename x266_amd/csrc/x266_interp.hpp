// x266_interp.hpp -- the sub-sample interpolation filters of include/x266hip.h (quarter-sample luma, eighth-sample 4:2:0 chroma),
// ONE copy of the taps and of the rounding for the motion compensation kernels and the quarter-sample refinement
// (subpel_kernels.hip).
//
// Every class of the header is the 2-D formula: row 0 of both tables is 64 at the centre tap and 0 elsewhere, so a stage with
// phase 0 multiplies by exactly 64 and the ">> 6" after the vertical stage takes it out again without loss --
//   fy = 0:  v = (64 h) >> 6 = h,            out = clip8((h + 32) >> 6)             the header's horizontal class
//   fx = 0:  h = 64 S, v = sum T S exactly,  out = clip8((sum T S + 32) >> 6)       the vertical class
//   both 0:  v = 64 S,                       out = (64 S + 32) >> 6 = S             the gather
// -- so the kernels run one code path and no lane branches on its class.
#pragma once

#include "x266_device.hpp"

namespace x266 {

constexpr uint64_t pack_taps(int a, int b, int c, int d, int e = 0, int f = 0, int g = 0, int h = 0)
{
    return (uint64_t)(uint8_t)a | (uint64_t)(uint8_t)b << 8 | (uint64_t)(uint8_t)c << 16 | (uint64_t)(uint8_t)d << 24 |
           (uint64_t)(uint8_t)e << 32 | (uint64_t)(uint8_t)f << 40 | (uint64_t)(uint8_t)g << 48 | (uint64_t)(uint8_t)h << 56;
}

// What differs between the planes: luma is 8 taps on bytes one apart at quarter-sample phases, chroma 4 taps on the (U, V) pairs of
// m_C -- bytes two apart -- at eighth-sample phases.  kBefore = taps in front of the sample.
template <bool CHROMA>
struct Interp {
    static constexpr int kTaps = CHROMA ? 4 : 8, kStride = CHROMA ? 2 : 1, kLog2Phases = CHROMA ? 3 : 2, kBefore = CHROMA ? 1 : 3;
};

// tap row f of the plane's table (a chain of selects on constants: no table in memory, no runtime-indexed array)
template <bool CHROMA>
__device__ __forceinline__ void interp_taps(int f, int (&t)[8])
{
    uint64_t p;
    if (CHROMA) {
        p = f == 0 ? pack_taps(0, 64, 0, 0) : f == 1 ? pack_taps(-2, 58, 10, -2) : f == 2 ? pack_taps(-4, 54, 16, -2) :
            f == 3 ? pack_taps(-6, 46, 28, -4) : f == 4 ? pack_taps(-4, 36, 36, -4) : f == 5 ? pack_taps(-4, 28, 46, -6) :
            f == 6 ? pack_taps(-2, 16, 54, -4) : pack_taps(-2, 10, 58, -2);
    } else {
        p = f == 0 ? pack_taps(0, 0, 0, 64, 0, 0, 0, 0) : f == 1 ? pack_taps(-1, 4, -10, 58, 17, -5, 1, 0) :
            f == 2 ? pack_taps(-1, 4, -11, 40, 40, -11, 4, -1) : pack_taps(0, 1, -5, 17, 58, -10, 4, -1);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = (int)(int8_t)(p >> (8 * k));
}

// The horizontal stage of one row: w holds the row's 16 bytes from the first tap of the first output on (little-endian dwords),
// h[c] = sum_k t[k] * byte[c + k * stride], unshifted, for the 8 outputs c of a row -- luma samples 0..7, or the interleaved
// (U, V) values of chroma pairs 0..3.  Luma reads bytes 0..14, chroma 0..13.
template <bool CHROMA>
__device__ __forceinline__ void interp_hsums(const uint32_t (&w)[4], const int (&t)[8], int (&h)[8])
{
    int b[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < Interp<CHROMA>::kTaps; ++k) s += t[k] * b[c + k * Interp<CHROMA>::kStride];
        h[c] = s;
    }
}

// The vertical stage of one sample, unrounded: col[k] = the horizontal sum of the row under tap k.  This is the header's
// intermediate V (luma -16830..33150, chroma -5897..22217: it does NOT fit int16), what bi-prediction averages.
template <bool CHROMA>
__device__ __forceinline__ int interp_vertical_v(const int (&col)[8], const int (&t)[8])
{
    int s = 0;
#pragma unroll
    for (int k = 0; k < Interp<CHROMA>::kTaps; ++k) s += t[k] * col[k];
    return s >> 6;                                                          // arithmetic: floors a negative sum
}

// The rounding of one sample from its unrounded V: clip8((V + 32) >> 6).
__device__ __forceinline__ int interp_round(int unrounded)
{
    const int v = unrounded + 32;
    // clip8(v >> 6) with the clamp in front of the shift: v >> 6 < 0 exactly when v < 0, > 255 exactly when v > 255 * 64 + 63.  (A
    // clamp behind the shift is what the compiler packs two results at a time with v_ashr_pk_u8_i32, which writes one half of its
    // destination and keeps the other: on an MI355X the kept half carried the bits of a negative sum into the neighbouring bytes.)
    return (v < 0 ? 0 : (v > 16383 ? 16383 : v)) >> 6;
}

// The vertical stage and the rounding of one sample.
template <bool CHROMA>
__device__ __forceinline__ int interp_vertical(const int (&col)[8], const int (&t)[8])
{
    return interp_round(interp_vertical_v<CHROMA>(col, t));
}

// The uni / bi combine of the header's x266_wp_t, ONE copy for the three bi-directional calls.  All three forms are
//   clip8((V0 * a0 + V1 * a1 + add) >> shift)
// with D = log2_denom + 6:   list 0 only  a0 = w0, a1 = 0,  add = 2^(D-1) + o0 * 2^D,      shift = D
//                            list 1 only  a0 = 0,  a1 = w1, add = 2^(D-1) + o1 * 2^D,      shift = D
//                            both         a0 = w0, a1 = w1, add = (o0 + o1 + 1) * 2^D,     shift = D + 1
// ("+ o" behind a ">> D" is "+ o * 2^D" in front of it, exactly).  |V * w| < 4.3e6 and |add| < 2^21: everything fits int32.
// comp = 0, 1, 2 for Y, U, V; dir = 1, 2, 3 as in d_dir.
struct BiTerms { int a0, a1, add, shift; };

__device__ __forceinline__ BiTerms bi_terms(const x266_wp_t &wp, int dir, int comp)
{
    const int D = (int)wp.log2_denom[comp != 0] + 6, w0 = wp.w[0][comp], w1 = wp.w[1][comp], o0 = wp.o[0][comp], o1 = wp.o[1][comp];
    BiTerms t;
    t.a0 = dir & 1 ? w0 : 0;
    t.a1 = dir & 2 ? w1 : 0;
    t.add = dir == 3 ? (o0 + o1 + 1) * (1 << D) : (1 << (D - 1)) + (dir & 1 ? o0 : o1) * (1 << D);
    t.shift = dir == 3 ? D + 1 : D;
    return t;
}
// the clamp in front of the shift, as in interp_vertical: x >> s < 0 exactly when x < 0, > 255 exactly when x > (256 << s) - 1
__device__ __forceinline__ int bi_round(int x, int shift)
{
    const int top = (256 << shift) - 1;
    return (x < 0 ? 0 : (x > top ? top : x)) >> shift;
}
__device__ __forceinline__ int bi_combine(const BiTerms &t, int v0, int v1) { return bi_round(v0 * t.a0 + v1 * t.a1 + t.add, t.shift); }

// eight horizontal sums (they fit int16: luma -6120..22440, chroma -2550..18870) as four dwords of pairs, and one of them back
__device__ __forceinline__ v4i pack_hsums(const int (&h)[8])
{
    return v4i{(int)((uint32_t)(h[0] & 0xFFFF) | (uint32_t)h[1] << 16), (int)((uint32_t)(h[2] & 0xFFFF) | (uint32_t)h[3] << 16),
               (int)((uint32_t)(h[4] & 0xFFFF) | (uint32_t)h[5] << 16), (int)((uint32_t)(h[6] & 0xFFFF) | (uint32_t)h[7] << 16)};
}
__device__ __forceinline__ int hsum_of(uint32_t pair, int odd) { return odd ? (int)pair >> 16 : (int)(pair << 16) >> 16; }

// LDS written by some lanes of a wave and read by others of the SAME wave: the wave's LDS instructions execute in order, so all
// this has to do is keep the compiler from moving the accesses across it.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace x266
