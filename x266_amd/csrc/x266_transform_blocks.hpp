// x266_transform_blocks.hpp -- the per-wave pieces of the mixed transform set's forward direction: a 32x32 tile of (32/N)^2 small
// blocks through the block-diagonal int8-MFMA pipeline of x266_mfma_blocks.hpp, the class's operand images built from the wave's LDS
// copy of the TileTab, a lane's row segment into a region's block-major layout, and the residual of a CTU's regions from two tiled
// frames.  Shared by transform_kernels.hip (the mixed-class tile kernel and the CTU kernels; the inverse direction stays there) and
// rdoq_kernels.hip (the transform decision): both run the same code on the same slot contents, so "the decision's coefficients are
// xTransformCtuFromTilesDev's" holds by construction.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"
#include "x266_mfma_blocks.hpp"
#include "x266_tables.hpp"

namespace x266 {

// One 32x32 tile of (32/N)^2 small blocks, block-major, sitting in a wave-private 2 KiB LDS slot: read the
// lane's fragment pieces, run the two MFMA passes with the class's operand images, write the results back
// in place.  Shared by the per-class kernels and the mixed-class tile kernel.
template <int LOGN>
__device__ __forceinline__ void fwd_tile_in_slot(unsigned char *slot, int lane, const LaneConsts &k)
{
    constexpr int N = 1 << LOGN;
    constexpr int PER = 32 / N, PIECES = N >= 16 ? 1 : 16 / N;
    constexpr int S1 = LOGN - 1, S2 = LOGN + 6;
    const int c = lane & 31, h = lane >> 5;
    const int row = c & (N - 1), tile_row = c >> LOGN;
    // byte offsets inside the 2 KiB tile of this lane's fragment pieces (block-major tile layout)
    unsigned frag[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const unsigned sb = N == 32 ? 0u : (unsigned)(tile_row * PER + h * PIECES + q);
        frag[q] = (sb * (unsigned)(N * N) + (unsigned)row * N + (N == 32 ? 16u * h : 0u)) * 2u;
    }
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        if (N >= 16) {
            const v4i a = *reinterpret_cast<const v4i *>(slot + frag[q]), b = *reinterpret_cast<const v4i *>(slot + frag[q] + 16);
            w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; w[4] = b[0]; w[5] = b[1]; w[6] = b[2]; w[7] = b[3];
        } else if (N == 8) {
            const v4i a = *reinterpret_cast<const v4i *>(slot + frag[q]);
            w[4 * q] = a[0]; w[4 * q + 1] = a[1]; w[4 * q + 2] = a[2]; w[4 * q + 3] = a[3];
        } else {
            const uint2 a = *reinterpret_cast<const uint2 *>(slot + frag[q]);
            w[2 * q] = a.x; w[2 * q + 1] = a.y;
        }
    }
    __builtin_amdgcn_wave_barrier();
    v4i r0, r1;
    fwd_block<S1, S2>(v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}, v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]}, k, r0, r1);
    const uint32_t z[8] = {(uint32_t)r0[0], (uint32_t)r0[1], (uint32_t)r0[2], (uint32_t)r0[3],
                           (uint32_t)r1[0], (uint32_t)r1[1], (uint32_t)r1[2], (uint32_t)r1[3]};
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        if (N >= 16) {
            *reinterpret_cast<v4i *>(slot + frag[q]) = r0;
            *reinterpret_cast<v4i *>(slot + frag[q] + 16) = r1;
        } else if (N == 8) {
            *reinterpret_cast<v4i *>(slot + frag[q]) = v4i{(int)z[4 * q], (int)z[4 * q + 1], (int)z[4 * q + 2], (int)z[4 * q + 3]};
        } else {
            *reinterpret_cast<uint2 *>(slot + frag[q]) = make_uint2(z[2 * q], z[2 * q + 1]);
        }
    }
}

// class byte of tile t through the scalar cache (uniform_byte, x266_device.hpp: t is wave-uniform), for any alignment of the table
__device__ __forceinline__ int tile_class_of(const uint8_t *__restrict__ tile_class, size_t t)
{
    return (int)(uniform_byte(tile_class, t) & 15u);
}

// Operand bytes B[16h + t][idx], t = 0..15, of blockdiag(M) given as rows: M[idx % N][(16h + t) % N] where the K-slot
// 16h + t lies in block idx / N, else 0.  `m` = the compact N x N matrix in LDS whose ROW idx % N holds those bytes.
template <int LOGN>
__device__ __forceinline__ v4i image_row_segment(const unsigned char *m, unsigned idx, unsigned h)
{
    constexpr unsigned N = 1u << LOGN;
    const unsigned rr = idx & (N - 1), b = idx >> LOGN;
    if constexpr (LOGN == 5) {
        return *reinterpret_cast<const v4i *>(m + rr * 32 + 16 * h);
    } else if constexpr (LOGN == 4) {                                    // K-slots 16h .. 16h+15 = block h
        const v4i v = *reinterpret_cast<const v4i *>(m + rr * 16);
        const int keep = b == h ? -1 : 0;
        return v4i{v[0] & keep, v[1] & keep, v[2] & keep, v[3] & keep};
    } else if constexpr (LOGN == 3) {                                    // dwords 0,1 = block 2h, dwords 2,3 = block 2h + 1
        const uint2 w = *reinterpret_cast<const uint2 *>(m + rr * 8);
        const int k0 = b == 2 * h ? -1 : 0, k1 = b == 2 * h + 1 ? -1 : 0;
        return v4i{(int)w.x & k0, (int)w.y & k0, (int)w.x & k1, (int)w.y & k1};
    } else {                                                             // dword q = block 4h + q
        const int w = *reinterpret_cast<const int *>(m + rr * 4);
        return v4i{b == 4 * h ? w : 0, b == 4 * h + 1 ? w : 0, b == 4 * h + 2 ? w : 0, b == 4 * h + 3 ? w : 0};
    }
}

// Forward pass 2: B[acc_row(t, h)][c], i.e. dword q holds columns 4h + 8q .. +3 of row c of blockdiag(M).
template <int LOGN>
__device__ __forceinline__ v4i image_acc_rows(const unsigned char *m, unsigned c, unsigned h)
{
    constexpr unsigned N = 1u << LOGN;
    const unsigned rr = c & (N - 1), b = c >> LOGN;
    if constexpr (LOGN == 5) {
        const int *q = reinterpret_cast<const int *>(m + rr * 32 + 4 * h);
        return v4i{q[0], q[2], q[4], q[6]};
    } else if constexpr (LOGN == 4) {                                    // columns 4h + 8q: block q >> 1, dword h + 2 (q & 1) of the row
        const int *q = reinterpret_cast<const int *>(m + rr * 16 + 4 * h);
        const int w0 = q[0], w1 = q[2];
        return v4i{b == 0 ? w0 : 0, b == 0 ? w1 : 0, b == 1 ? w0 : 0, b == 1 ? w1 : 0};
    } else if constexpr (LOGN == 3) {                                    // block q, dword h of the row
        const int w = *reinterpret_cast<const int *>(m + rr * 8 + 4 * h);
        return v4i{b == 0 ? w : 0, b == 1 ? w : 0, b == 2 ? w : 0, b == 3 ? w : 0};
    } else {                                                             // block h + 2q, the row's one dword
        const int w = *reinterpret_cast<const int *>(m + rr * 4);
        return v4i{b == h ? w : 0, b == h + 2 ? w : 0, b == h + 4 ? w : 0, b == h + 6 ? w : 0};
    }
}

// tab: the wave's LDS copy of the TileTab; hs / vs: the slots (0 / 1) of the class's horizontal and vertical transform
template <int LOGN>
__device__ __forceinline__ void fwd_tile_of_class(unsigned char *slot, const unsigned char *tab, int lane, unsigned hs, unsigned vs)
{
    asm volatile("" : "+v"(lane));          // per-size lane arithmetic stays inside its branch: hoisted out of the four-way switch (x 2 tiles) it costs registers
    constexpr unsigned N = 1u << LOGN;
    constexpr int S1 = LOGN - 1, S2 = LOGN + 6;
    const unsigned c = lane & 31, h = lane >> 5, kc = (unsigned)kappa((int)c);
    const unsigned mh = tile_tab_mat(0, LOGN - 2) + (LOGN == 5 ? 0u : hs * 336u), mv = tile_tab_mat(0, LOGN - 2) + (LOGN == 5 ? 0u : vs * 336u);
    const unsigned sh = tile_tab_sum(0, LOGN - 2) + (LOGN == 5 ? 0u : hs * 112u), sv = tile_tab_sum(0, LOGN - 2) + (LOGN == 5 ? 0u : vs * 112u);
    LaneConsts k;
    k.p1 = image_row_segment<LOGN>(tab + mh, kc, h);                     // pass 1: M[kappa(c)][16h + t]
    k.p2 = image_acc_rows<LOGN>(tab + mv, c, h);                         // pass 2: M[c][acc_row(t, h)]
    k.tr = v4i{0, 0, 0, 0};
    k.c1 = (1 << (S1 - 1)) + reinterpret_cast<const int *>(tab + sh)[kc & (N - 1)];
    k.c2 = (1 << (S2 - 1)) + reinterpret_cast<const int *>(tab + sv)[c & (N - 1)];
    fwd_tile_in_slot<LOGN>(slot, lane, k);
}

// the slots (0 / 1) of a class's horizontal and vertical transform: type 0 DCT-II, 1 DST-VII, 2 h = slot 1 / v = slot 0, 3 the other
// way (wave-uniform)
__device__ __forceinline__ unsigned class_h_slot(int cls) { const unsigned type = (unsigned)cls >> 2; return (type == 1 || type == 2) ? 1u : 0u; }
__device__ __forceinline__ unsigned class_v_slot(int cls) { const unsigned type = (unsigned)cls >> 2; return (type == 1 || type == 3) ? 1u : 0u; }

// the forward transform of the slot's tile for a wave-uniform class byte (what tile_of_class<false> of transform_kernels.hip runs)
__device__ __forceinline__ void fwd_tile_of_any_class(unsigned char *slot, const unsigned char *tab, int lane, int cls)
{
    const unsigned hs = class_h_slot(cls), vs = class_v_slot(cls);
    switch (cls & 3) {
    case 0: fwd_tile_of_class<2>(slot, tab, lane, hs, vs); break;
    case 1: fwd_tile_of_class<3>(slot, tab, lane, hs, vs); break;
    case 2: fwd_tile_of_class<4>(slot, tab, lane, hs, vs); break;
    default: fwd_tile_of_class<5>(slot, tab, lane, hs, vs); break;
    }
}

// ---- a region's row segments ------------------------------------------------------------------------------------------------------
// Lane (c, h) holds row c, columns 16h .. 16h+15 of a region, and in the block-major layout of every class those 16 samples are whole
// runs: one 32-byte run (N = 32, 16), two of 16 bytes (N = 8) or four of 8 bytes (N = 4) -- exactly the fragment pieces
// fwd_tile_in_slot reads.

// byte offset in a region's block-major layout of run p of lane (c, h)'s row segment (N = 1 << LOGN, 16 / N runs for N < 16)
template <int LOGN>
__device__ __forceinline__ unsigned segment_run(unsigned c, unsigned h, unsigned p)
{
    constexpr unsigned N = 1u << LOGN;
    const unsigned sb = (c >> LOGN) * (32u >> LOGN) + ((16u * h + p * N) >> LOGN);
    return (sb * N * N + (c & (N - 1)) * N + (LOGN == 5 ? 16u * h : 0u)) * 2u;
}

// d = 16 int16 samples of the row segment as pairs, in column order
template <int LOGN>
__device__ __forceinline__ void put_segment_of(unsigned char *slot, unsigned c, unsigned h, const uint32_t (&d)[8])
{
    if constexpr (LOGN >= 4) {
        unsigned char *p = slot + segment_run<LOGN>(c, h, 0);
        *reinterpret_cast<v4i *>(p) = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
        *reinterpret_cast<v4i *>(p + 16) = v4i{(int)d[4], (int)d[5], (int)d[6], (int)d[7]};
    } else if constexpr (LOGN == 3) {
#pragma unroll
        for (unsigned p = 0; p < 2; ++p)
            *reinterpret_cast<v4i *>(slot + segment_run<3>(c, h, p)) = v4i{(int)d[4 * p], (int)d[4 * p + 1], (int)d[4 * p + 2], (int)d[4 * p + 3]};
    } else {
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) *reinterpret_cast<uint2 *>(slot + segment_run<2>(c, h, p)) = make_uint2(d[2 * p], d[2 * p + 1]);
    }
}

// the class is wave-uniform: one branch per region
__device__ __forceinline__ void put_segment(unsigned char *slot, int cls, unsigned c, unsigned h, const uint32_t (&d)[8])
{
    switch (cls & 3) {
    case 0: put_segment_of<2>(slot, c, h, d); break;
    case 1: put_segment_of<3>(slot, c, h, d); break;
    case 2: put_segment_of<4>(slot, c, h, d); break;
    default: put_segment_of<5>(slot, c, h, d); break;
    }
}

// ---- the residual of a CTU's regions from two tiled frames -----------------------------------------------------------------------
__device__ __forceinline__ uint32_t sub_pairs(uint32_t x, uint32_t z)    // two 9-bit residuals, v_pk_sub_i16
{
    typedef short v2s __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(v2s, x) - __builtin_bit_cast(v2s, z));
}

// 16 luma residuals of one tile row: cur - pred, pixel order
__device__ __forceinline__ void luma_residual16(const v4i &a, const v4i &b, uint32_t (&d)[8])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (uint32_t)a[q], z = (uint32_t)b[q];
        d[2 * q] = sub_pairs(bperm(0u, x, 0x0c010c00u), bperm(0u, z, 0x0c010c00u));
        d[2 * q + 1] = sub_pairs(bperm(0u, x, 0x0c030c02u), bperm(0u, z, 0x0c030c02u));
    }
}

// 8 U and 8 V residuals of one m_C row (u v u v ...): even bytes U, odd bytes V
__device__ __forceinline__ void chroma_residual8(const v4i &a, const v4i &b, uint32_t *du, uint32_t *dv)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (uint32_t)a[q], z = (uint32_t)b[q];
        du[q] = sub_pairs(x & 0x00FF00FFu, z & 0x00FF00FFu);
        dv[q] = sub_pairs((x >> 8) & 0x00FF00FFu, (z >> 8) & 0x00FF00FFu);
    }
}

struct CtuPlace {
    size_t cy, cx;
    int tiles_x, tiles_y;
    __device__ bool luma_in(unsigned part) const { return ctu_luma_tile_col(cx, part, 0) < (size_t)tiles_x && ctu_luma_tile_row(cy, part, 0) < (size_t)tiles_y; }
};

// the wave's LDS copy of the TileTab (2 KiB): two 16-byte loads per lane
__device__ __forceinline__ void copy_table(unsigned char *tab, const TileTab *__restrict__ T, int lane)
{
    const char *src = reinterpret_cast<const char *>(T->b) + lane * 16;
    const v4i q0 = *reinterpret_cast<const v4i *>(src), q1 = *reinterpret_cast<const v4i *>(src + 1024);
    *reinterpret_cast<v4i *>(tab + lane * 16) = q0;
    *reinterpret_cast<v4i *>(tab + 1024 + lane * 16) = q1;
}

}  // namespace x266
