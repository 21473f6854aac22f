// x266_mfma_blocks.hpp -- device-side building blocks shared by the transform kernels:
// byte-plane split / re-pack around v_mfma_i32_32x32x32_i8, the two-pass forward transform of one
// 32x32 tile held in registers (fwd_block; fwd_from_pixels for 8-bit cur / pred rows, chroma_plane
// for their U,V de-interleave; their steps pixels_pass1, pass1_planes, fwd_pass2, and the other operand
// orientation fwd_pass2_swapped of the CTU coding kernel, which feeds an inverse from registers), the inverse's passes
// with their constants and column gather
// (inv_passes, load_c2r, column_base / read_column_planes), the wave-private LDS slot as layout
// converter (lds_slot, TileLanes, frag_to_linear, fwd_tile_staged) and the reconstruction into pixels
// (recon_luma16 / recon_chroma16).  See dct32_kernels.hip for the derivation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_tables.hpp"

namespace x266 {

// ---- byte-plane helpers ----------------------------------------------------
// v_perm_b32: result byte i = byte sel[i] of the 8-byte value {hi_src, lo_src}
// (indices 0-3 = lo_src, 4-7 = hi_src).
__device__ __forceinline__ uint32_t bperm(uint32_t hi_src, uint32_t lo_src, uint32_t sel)
{
    return __builtin_amdgcn_perm(hi_src, lo_src, sel);
}

// 8 dwords of int16 pairs -> 4 dwords of low bytes (offset to signed) + 4 of high bytes
__device__ __forceinline__ void split_planes(const v4i &w0, const v4i &w1, v4i &lo, v4i &hi)
{
    const uint32_t w[8] = {(uint32_t)w0[0], (uint32_t)w0[1], (uint32_t)w0[2], (uint32_t)w0[3],
                           (uint32_t)w1[0], (uint32_t)w1[1], (uint32_t)w1[2], (uint32_t)w1[3]};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        lo[p] = (int)(bperm(w[2 * p + 1], w[2 * p], 0x06040200u) ^ 0x80808080u);
        hi[p] = (int)bperm(w[2 * p + 1], w[2 * p], 0x07050301u);
    }
}

// 16 int32 whose bytes 0/1 hold the wanted low/high byte -> byte planes
__device__ __forceinline__ void pack_planes(const v16i &s, v4i &lo, v4i &hi)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t t01 = bperm((uint32_t)s[4 * q + 1], (uint32_t)s[4 * q + 0], 0x05010400u);
        const uint32_t t23 = bperm((uint32_t)s[4 * q + 3], (uint32_t)s[4 * q + 2], 0x05010400u);
        lo[q] = (int)(bperm(t23, t01, 0x05040100u) ^ 0x80808080u);
        hi[q] = (int)bperm(t23, t01, 0x07060302u);
    }
}

// 16 int32 holding one signed byte value each (byte 0) -> one plane of 4 dwords
__device__ __forceinline__ v4i pack_bytes(const v16i &s)
{
    v4i r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t t01 = bperm((uint32_t)s[4 * q + 1], (uint32_t)s[4 * q + 0], 0x0c0c0400u);
        const uint32_t t23 = bperm((uint32_t)s[4 * q + 3], (uint32_t)s[4 * q + 2], 0x0c0c0400u);
        r[q] = (int)bperm(t23, t01, 0x05040100u);
    }
    return r;
}

__device__ __forceinline__ v16i mfma(const v4i &a, const v4i &b, const v16i &c)
{
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
}

struct LaneConsts {
    v4i p1, p2, tr;
    int c1, c2;
};

__device__ __forceinline__ LaneConsts load_consts(const DctOps *ops, int lane)
{
    LaneConsts k;
    const DctLaneOps *r = &ops->lane[lane];
    k.p1 = *reinterpret_cast<const v4i *>(r->p1);
    k.p2 = *reinterpret_cast<const v4i *>(r->p2);
    k.tr = *reinterpret_cast<const v4i *>(r->tr);
    k.c1 = r->c1;
    k.c2 = r->c2;
    return k;
}

// ---- forward: one block held as (w0, w1) -> (o0, o1) ------------------------
// the pass-1 sums (rounding term included) shifted and re-packed to the byte planes pass 2 takes
template <int S1>
__device__ __forceinline__ void pass1_planes(v16i acc, v4i &ylo, v4i &yhi)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc[r] >> S1;        // bytes 0/1 = int16 result
    pack_planes(acc, ylo, yhi);
}

// pass 2 (columns), natural orientation: data = A (pass-1 accumulators re-packed), coefficients = B.  The sums before the final
// shift: 16 consecutive coefficients of one output row per lane.
__device__ __forceinline__ v16i fwd_pass2(const v4i &ylo, const v4i &yhi, const LaneConsts &k)
{
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i acc = mfma(yhi, k.p2, zero);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = (int)(((uint32_t)acc[r] << 8) + (uint32_t)k.c2);
    return mfma(ylo, k.p2, acc);
}

// pass 2 in the OTHER operand orientation (coefficients = A, data = B; dct32_kernels.hip, "fused forward + inverse"): lane (i, h)
// gets the sums Z[acc_row(r, h)][kappa(i)] of the 32-point DCT-II with final shift 11 -- sixteen rows of one column, the A
// fragment of the inverse's first contraction in accumulator-row order.  The byte-plane offset fix belongs to output row 0 =
// accumulator register 0 of the lower half-wave.  dct32_fwdinv_kernel keeps its own inline form of this pass: its loop is scheduled
// around hand-counted waits and hoists the offset constant, and it is left exactly as measured.
__device__ __forceinline__ v16i fwd_pass2_swapped(const v4i &ylo, const v4i &yhi, const LaneConsts &k, unsigned h)
{
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i acc = mfma(k.p2, yhi, zero);
    acc[0] = (int)(((uint32_t)acc[0] << 8) + (uint32_t)((1 << 10) + (h ? 0 : 128 * 2048)));
#pragma unroll
    for (int r = 1; r < 16; ++r) acc[r] = (int)(((uint32_t)acc[r] << 8) + (1u << 10));
    return mfma(k.p2, ylo, acc);
}

// Second half of the forward transform: `acc` holds the pass-1 sums INCLUDING the rounding term;
// shift, re-pack to byte planes, pass 2, final shift and int16 packing.
template <int S1, int S2>
__device__ __forceinline__ void fwd_finish(v16i acc, const LaneConsts &k, v4i &o0, v4i &o1)
{
    v4i ylo, yhi;
    pass1_planes<S1>(acc, ylo, yhi);
    acc = fwd_pass2(ylo, yhi, k);

    // (acc >> S2) truncated to int16, pairs packed into dwords
    uint32_t z[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        z[m] = bperm((uint32_t)(acc[2 * m + 1] >> S2), (uint32_t)(acc[2 * m] >> S2), 0x05040100u);
    o0 = v4i{(int)z[0], (int)z[1], (int)z[2], (int)z[3]};
    o1 = v4i{(int)z[4], (int)z[5], (int)z[6], (int)z[7]};
}

template <int S1, int S2>
__device__ __forceinline__ void fwd_block(const v4i &w0, const v4i &w1, const LaneConsts &k,
                                          v4i &o0, v4i &o1)
{
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v4i lo, hi;
    split_planes(w0, w1, lo, hi);

    // pass 1 (rows): data = A, coefficients = B
    v16i acc = mfma(hi, k.p1, zero);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = (int)(((uint32_t)acc[r] << 8) + (uint32_t)k.c1);
    acc = mfma(lo, k.p1, acc);
    fwd_finish<S1, S2>(acc, k, o0, o1);
}

// The forward transform of cur - pred on 8-bit pixels as they are (dct32_kernels.hip, "fused residual + forward transform"):
// pass 1 is G*cur + (-G)*pred, ONE byte plane per frame, the +128 of the (x ^ 0x80) signed-offset trick cancels and the
// rounding constant is the MFMA's inline C operand.  a / b: the lane's 16 cur / pred pixels (row c, columns 16h .. 16h+15).
__device__ __forceinline__ v16i pixels_pass1(const v4i &a, const v4i &b, const LaneConsts &k)
{
    const v4i bias = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};
    const v16i round1 = {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8};
    const v16i acc = mfma(a ^ bias, k.p1, round1);
    return mfma(b ^ bias, k.tr, acc);                         // k.tr = -p1 in the forward tables
}

__device__ __forceinline__ void fwd_from_pixels(const v4i &a, const v4i &b, const LaneConsts &k, v4i &o0, v4i &o1)
{
    fwd_finish<4, 11>(pixels_pass1(a, b, k), k, o0, o1);
}

// One chroma plane's 16 pixels out of two m_C lines (8 interleaved U,V pairs each): sel = kSelU / kSelV
constexpr uint32_t kSelU = 0x06040200u, kSelV = 0x07050301u;       // even bytes = U, odd bytes = V
__device__ __forceinline__ v4i chroma_plane(const v4i &a0, const v4i &a1, uint32_t sel)
{
    return v4i{(int)bperm((uint32_t)a0[1], (uint32_t)a0[0], sel), (int)bperm((uint32_t)a0[3], (uint32_t)a0[2], sel),
               (int)bperm((uint32_t)a1[1], (uint32_t)a1[0], sel), (int)bperm((uint32_t)a1[3], (uint32_t)a1[2], sel)};
}

// ---- one 32x32 tile through a wave-private 2 KiB LDS slot (dct32_kernels.hip, "LDS-staged variant") ----------
// Chunk (row r, quarter q) lives at r*64 + ((q ^ ((r >> 2) & 3)) << 4): linear writes, row-per-lane fragment reads and
// the way back are all bank-conflict-free.
__device__ __forceinline__ unsigned lds_slot(unsigned row, unsigned quarter)
{
    return row * 64u + ((quarter ^ ((row >> 2) & 3u)) << 4);
}

// A lane's four 16-byte chunks of a slot: lin0 / lin1 = its pieces of the tile in LINEAR order (bytes lane*16 and 1024 + lane*16, what a
// 1 KiB-linear global instruction moves), frag0 / frag1 = its fragment, row (lane & 31), columns 16 (lane >> 5) .. +15.
struct TileLanes {
    unsigned lin0, lin1, frag0, frag1;
};
__device__ __forceinline__ TileLanes tile_lanes(int lane)
{
    const unsigned c = lane & 31, h = lane >> 5;
    return {lds_slot(lane >> 2, lane & 3), lds_slot(16 + (lane >> 2), lane & 3), lds_slot(c, 2 * h), lds_slot(c, 2 * h + 1)};
}

// the slot as layout converter on the way out: fragments (o0, o1) in, the same tile's linear pieces (s0, s1) out.  The barriers that
// order this against the slot's previous and next use are the caller's.
__device__ __forceinline__ void frag_to_linear(unsigned char *slot, const TileLanes &t, const v4i &o0, const v4i &o1, v4i &s0, v4i &s1)
{
    *reinterpret_cast<v4i *>(slot + t.frag0) = o0;
    *reinterpret_cast<v4i *>(slot + t.frag1) = o1;
    __builtin_amdgcn_wave_barrier();
    s0 = *reinterpret_cast<const v4i *>(slot + t.lin0);
    s1 = *reinterpret_cast<const v4i *>(slot + t.lin1);
}

// g0 / g1: the lane's two linear pieces of the tile; returns the transformed tile's pieces in the same linear order.
template <int S1, int S2>
__device__ __forceinline__ void fwd_tile_staged(unsigned char *slot, int lane, const LaneConsts &k, const v4i &g0, const v4i &g1, v4i &s0, v4i &s1)
{
    const TileLanes t = tile_lanes(lane);
    *reinterpret_cast<v4i *>(slot + t.lin0) = g0;
    *reinterpret_cast<v4i *>(slot + t.lin1) = g1;
    __builtin_amdgcn_wave_barrier();
    const v4i a0 = *reinterpret_cast<const v4i *>(slot + t.frag0);
    const v4i a1 = *reinterpret_cast<const v4i *>(slot + t.frag1);
    v4i o0, o1;
    fwd_block<S1, S2>(a0, a1, k, o0, o1);
    __builtin_amdgcn_wave_barrier();
    frag_to_linear(slot, t, o0, o1, s0, s1);
    __builtin_amdgcn_wave_barrier();
}

// ---- inverse passes (see dct32_kernels.hip, section "inverse") --------------------------------

// {clip16(lo), clip16(hi)} packed into one dword: v_cvt_pk_i16_i32 (full rate, profiles/r01_alubench.txt)
__device__ __forceinline__ uint32_t sat_pack16(int lo, int hi)
{
    typedef short v2s __attribute__((ext_vector_type(2)));
    const v2s r = __builtin_amdgcn_cvt_pk_i16(lo, hi);
    return __builtin_bit_cast(uint32_t, r);
}

// passes A and B on column data: zlo / zhi = byte planes of 16 samples of ONE COLUMN per lane.
// c2r_group(g): the pass-B constants of accumulator registers 4g .. 4g+3 (fetched where they are used: four live, not sixteen)
template <class C2RGroup>
__device__ __forceinline__ void inv_passes_with(const v4i &zlo, const v4i &zhi, const LaneConsts &k,
                                                C2RGroup c2r_group, v4i &o0, v4i &o1)
{
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // pass A (columns): data = A, coefficients = B, per-lane constant
    v16i acc = mfma(zhi, k.p1, zero);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = (int)(((uint32_t)acc[r] << 8) + (uint32_t)k.c1);
    acc = mfma(zlo, k.p1, acc);
    // shift, clip to int16 and re-pack to byte planes: v_cvt_pk_i16_i32 saturates and packs two
    // values per instruction (instead of two v_med3 + byte shuffles on 32-bit values)
    v4i tlo2, thi2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t p01 = sat_pack16(acc[4 * q + 0] >> 7, acc[4 * q + 1] >> 7);
        const uint32_t p23 = sat_pack16(acc[4 * q + 2] >> 7, acc[4 * q + 3] >> 7);
        tlo2[q] = (int)(bperm(p23, p01, 0x06040200u) ^ 0x80808080u);
        thi2[q] = (int)bperm(p23, p01, 0x07050301u);
    }

    // pass B (rows): coefficients = A, data = B, per-register constant
    acc = mfma(k.p2, thi2, zero);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const v4i c = c2r_group(g);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * g + i] = (int)(((uint32_t)acc[4 * g + i] << 8) + (uint32_t)c[i]);
    }
    acc = mfma(k.p2, tlo2, acc);

    uint32_t z[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) z[m] = sat_pack16(acc[2 * m] >> 12, acc[2 * m + 1] >> 12);
    o0 = v4i{(int)z[0], (int)z[1], (int)z[2], (int)z[3]};
    o1 = v4i{(int)z[4], (int)z[5], (int)z[6], (int)z[7]};
}

__device__ __forceinline__ void inv_passes(const v4i &zlo, const v4i &zhi, const LaneConsts &k,
                                           const v16i &c2r, v4i &o0, v4i &o1)
{
    inv_passes_with(zlo, zhi, k, [&](int g) { return v4i{c2r[4 * g], c2r[4 * g + 1], c2r[4 * g + 2], c2r[4 * g + 3]}; }, o0, o1);
}

// the pass-B constants depend on (half, register) only: two scalar loads (wave-uniform addresses) and a per-lane select
// instead of 64 bytes of vector loads per lane and wave
__device__ __forceinline__ v16i load_c2r(const DctOps *__restrict__ ops, int h)
{
    const int *__restrict__ s0 = ops->c2r[0], *__restrict__ s1 = ops->c2r[32];
    v16i c2r;
#pragma unroll
    for (int r = 0; r < 16; ++r) c2r[r] = h ? s1[r] : s0[r];
    return c2r;
}

// The inverse contracts over the block's ROW index first: with the tile staged in a slot (lds_slot layout) lane (c, h) simply reads
// its COLUMN u = kappa(c), rows 16h .. 16h+15.  Byte offset of element (row 16h + t, column u): base[(t >> 2) & 3] + 64 t.
__device__ __forceinline__ void column_base(unsigned c, unsigned h, unsigned (&base)[4])
{
    const unsigned u = (unsigned)kappa((int)c);
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) base[j] = 16u * h * 64u + ((((u >> 3) ^ j) & 3u) << 4) + (u & 7u) * 2u;
}

// 16 x ds_read_u16 down the lane's column, then the byte planes inv_passes takes
__device__ __forceinline__ void read_column_planes(const unsigned char *slot, const unsigned (&base)[4], v4i &lo, v4i &hi)
{
    uint32_t w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const uint32_t e0 = *reinterpret_cast<const uint16_t *>(slot + base[((2 * m) >> 2) & 3] + (2 * m) * 64);
        const uint32_t e1 = *reinterpret_cast<const uint16_t *>(slot + base[((2 * m + 1) >> 2) & 3] + (2 * m + 1) * 64);
        w[m] = e0 | (e1 << 16);
    }
    split_planes(v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}, v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]}, lo, hi);
}

// ---- reconstruction: clip8(pred + residual), exact for every int16 residual --------------------------------------------------
// Two pixels per 16-bit lane pair: v_pk_add_i16 with clamp saturates pred (0..255) + residual to int16, which never moves the
// result across the 0 / 255 bounds, then v_pk_max_i16 / v_pk_min_i16 clip it to 0..255 (a wrapping add would turn 100 + 32767
// into a negative number).  `p` holds the two pred bytes zero-extended to 16 bits, `r` the two int16 residuals.
__device__ __forceinline__ uint32_t add_clip8x2(uint32_t p, uint32_t r)
{
    typedef short v2i16 __attribute__((ext_vector_type(2)));
    const v2i16 lo = {0, 0}, hi = {255, 255};
    const v2i16 s = __builtin_elementwise_add_sat(__builtin_bit_cast(v2i16, p), __builtin_bit_cast(v2i16, r));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(s, lo), hi));
}

// 16 luma pixels: p = 16 pred bytes, r0 / r1 = residuals 0..7 / 8..15 as int16 pairs in column order
__device__ __forceinline__ v4i recon_luma16(const v4i &p, const v4i &r0, const v4i &r1)
{
    const uint32_t r[8] = {(uint32_t)r0[0], (uint32_t)r0[1], (uint32_t)r0[2], (uint32_t)r0[3],
                           (uint32_t)r1[0], (uint32_t)r1[1], (uint32_t)r1[2], (uint32_t)r1[3]};
    v4i o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (uint32_t)p[q];
        const uint32_t s01 = add_clip8x2(bperm(0u, x, 0x0c010c00u), r[2 * q]);      // pixels 4q, 4q+1 (sel 0x0c = zero byte)
        const uint32_t s23 = add_clip8x2(bperm(0u, x, 0x0c030c02u), r[2 * q + 1]);  // pixels 4q+2, 4q+3
        o[q] = (int)bperm(s23, s01, 0x06040200u);
    }
    return o;
}

// 8 interleaved (U, V) chroma pairs of m_C: p = 16 pred bytes u0 v0 u1 v1 ..., ru / rv = the 8 U / 8 V residuals as int16 pairs
__device__ __forceinline__ v4i recon_chroma16(const v4i &p, const v4i &ru, const v4i &rv)
{
    v4i o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (uint32_t)p[q];                                                  // u(2q) v(2q) u(2q+1) v(2q+1)
        const uint32_t su = add_clip8x2(bperm(0u, x, 0x0c020c00u), (uint32_t)ru[q]);
        const uint32_t sv = add_clip8x2(bperm(0u, x, 0x0c030c01u), (uint32_t)rv[q]);
        o[q] = (int)bperm(sv, su, 0x06020400u);                                            // re-interleave
    }
    return o;
}

}  // namespace x266
