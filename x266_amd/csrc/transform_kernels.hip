// transform_kernels.hip -- forward DCT-II 4/8/16 and DST-VII 4/8/16 for gfx950
// (BASELINE configs[3]: the mixed transform set: DCT-II + closed-form DST-VII, or caller-supplied matrices).
//
// Reference anchor: the N-point DCT-II matrices are sub-matrices of g_t32
// (src_tb/dct32.c:30-64; the RTL re-uses the adder-tree taps for 4/8/16,
// src/mkDct32.bsv:132-141) and the pass structure / rounding / truncating store
// are partialButterfly32's (src_tb/dct32.c:66-170) with shifts log2N-1 and
// log2N+6.  Upstream has no C model for these sizes nor any DST-VII: parity is
// UNPINNED and rests on the CPU statement kept with the tests.
//
// Mapping: (32/N)^2 small blocks form one 32x32 tile; transforming the tile with
// the block-diagonal matrix diag(M_N,...) on both sides transforms every small
// block on its own.  The tile runs through exactly the two-pass int8-MFMA
// pipeline of dct32_kernels.hip (x266_mfma_blocks.hpp); only the lane -> address
// pattern and the operand images differ.  Blocks are N x N int16 row-major and
// either contiguous (block b at b*N*N samples) or placed by a per-block offset
// table (the mixed per-CTU batches of configs[3]).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"
#include "x266_mfma_blocks.hpp"
#include "x266_tables.hpp"
#include "x266_transform_blocks.hpp"

namespace x266 {
namespace {

// The forward tile pipeline (fwd_tile_in_slot, the operand images, fwd_tile_of_class), a region's row segments (put_segment), the
// residual of a CTU's regions and the table copy are x266_transform_blocks.hpp's: rdoq_kernels.hip's transform decision runs them too.

// A tile's (32/N)^2 blocks are 2 KiB of consecutive memory (contiguous batches) or (32/N)^2 pieces placed by the
// offset table, moved with linear 1 KiB instructions (whole 128-byte lines per instruction, see
// dct32_kernels.hip section "LDS-staged variant") and re-read from a wave-private LDS slot in
// fragment order.  Streaming cache hints only for contiguous batches: scattered blocks may share lines across instructions.
template <int LOGN, bool INDEXED>
__device__ __forceinline__ void tr_fwd_small_body(unsigned char *stage, size_t wave, const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                  size_t n_blocks, const DctOps *__restrict__ ops,
                                                  const uint32_t *__restrict__ offsets, unsigned tiles_per_wave)
{
    constexpr int N = 1 << LOGN;
    constexpr int PER = 32 / N, NSB = PER * PER;
    unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;

    const int lane = threadIdx.x & 63;
    const size_t n_tiles = (n_blocks + NSB - 1) / NSB;
    size_t t = wave * tiles_per_wave;
    const size_t t_end = t + tiles_per_wave < n_tiles ? t + tiles_per_wave : n_tiles;
    if (t >= t_end) return;
    const LaneConsts k = load_consts(ops, lane);
    const size_t total_bytes = n_blocks * (size_t)(N * N * 2);
    for (; t < t_end; ++t) {
        size_t o0, o1;
        bool live0, live1;
        if (INDEXED) {
            // chunk c (16 bytes) of the tile belongs to block c / CPB of the tile, placed by the offset table:
            // blocks that sit next to each other in memory still make line-dense instructions
            constexpr int CPB = N * N / 8;                               // 16-byte chunks per block
            size_t b0 = t * NSB + (size_t)(lane / CPB), b1 = t * NSB + (size_t)((lane + 64) / CPB);
            live0 = b0 < n_blocks;
            live1 = b1 < n_blocks;
            if (!live0) b0 = n_blocks - 1;                               // ragged tail: re-read the last block
            if (!live1) b1 = n_blocks - 1;
            o0 = ((size_t)offsets[b0] * 2) + (size_t)(lane % CPB) * 16;
            o1 = ((size_t)offsets[b1] * 2) + (size_t)((lane + 64) % CPB) * 16;
        } else {
            const size_t base = t * 2048;
            o0 = base + (size_t)lane * 16;
            o1 = o0 + 1024;
            live0 = o0 + 16 <= total_bytes;
            live1 = o1 + 16 <= total_bytes;
            if (!live0) o0 = total_bytes - 16;                           // ragged tail: stay inside the buffer
            if (!live1) o1 = total_bytes - 16;
        }
        const v4i g0 = load16<true>(reinterpret_cast<const char *>(in) + o0);   // streaming hints, offset tables included (round 5: -8 % on the per-class calls over a CTU-ordered buffer, profiles/r05_result_stores.txt)
        const v4i g1 = load16<true>(reinterpret_cast<const char *>(in) + o1);
        *reinterpret_cast<v4i *>(slot + lane * 16) = g0;
        *reinterpret_cast<v4i *>(slot + 1024 + lane * 16) = g1;
        __builtin_amdgcn_wave_barrier();
        fwd_tile_in_slot<LOGN>(slot, lane, k);
        __builtin_amdgcn_wave_barrier();
        const v4i s0 = *reinterpret_cast<const v4i *>(slot + lane * 16);
        const v4i s1 = *reinterpret_cast<const v4i *>(slot + 1024 + lane * 16);
        __builtin_amdgcn_wave_barrier();
        if (live0) store16m<2>(reinterpret_cast<char *>(out) + o0, s0);   // "sc1 nt" (x266_device.hpp)
        if (live1) store16m<2>(reinterpret_cast<char *>(out) + o1, s1);
    }
}

// One kernel per size: the offset-table form and the contiguous form are two complete bodies (each with its own addressing AND cache
// policy at compile time) behind one wave-uniform test of the kernel argument.  A run-time choice INSIDE the loop costs 1-3.6 %; this
// form measures +-0.3 % on the forward family, +0.5-1 % FASTER on the tile kernel below and, once the inverse family's column gather
// is pinned pair by pair (inv_tile_in_slot_with<.., PAIRWISE>: left alone, the merged function issues the sixteen reads as one burst,
// 0.5-1.9 % slower), +0.1-1 % on the contiguous inverse family -- profiles/r04_kernel_prune.txt.  (32x32 exists only in the offset-table form:
// contiguous 32x32 batches are dct32_kernels.hip's.)
template <int LOGN>
__global__ __launch_bounds__(256) void tr_fwd_small_lds_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                               size_t n_blocks, const DctOps *__restrict__ ops,
                                                               const uint32_t *__restrict__ offsets, unsigned tiles_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];   // 2 KiB per wave (+ occupancy padding)
    // everything both bodies need from the dispatch packet is read BEFORE the branch (a scalar load issued behind it would be a second
    // round trip in every wave's prologue)
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (LOGN == 5 || offsets) tr_fwd_small_body<LOGN, true>(stage, wave, in, out, n_blocks, ops, offsets, tiles_per_wave);
    else                      tr_fwd_small_body<LOGN, LOGN == 5>(stage, wave, in, out, n_blocks, ops, offsets, tiles_per_wave);
}

// The inverse of fwd_tile_in_slot: the first contraction runs over the tile's ROW index, so each lane reads
// its COLUMN out of the staged tile (16 x ds_read_u16), exactly as the staged DCT32 inverse does.
template <int LOGN, class C2RGroup, bool PAIRWISE = false>
__device__ __forceinline__ void inv_tile_in_slot_with(unsigned char *slot, int lane, const LaneConsts &k, C2RGroup c2r_group)
{
    constexpr int N = 1 << LOGN;
    constexpr int PER = 32 / N, PIECES = N >= 16 ? 1 : 16 / N;
    const int c = lane & 31, h = lane >> 5;
    const int row = c & (N - 1), tile_row = c >> LOGN;
    unsigned frag[PIECES];                                              // output fragment pieces (as in the forward body)
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const unsigned sb = N == 32 ? 0u : (unsigned)(tile_row * PER + h * PIECES + q);
        frag[q] = (sb * (unsigned)(N * N) + (unsigned)row * N + (N == 32 ? 16u * h : 0u)) * 2u;
    }
    // input column u = kappa(c), rows v = 16h + t: byte offset = col_base + ((t / N) * 64 * N + (t % N) * 2 * N)
    const unsigned u = (unsigned)kappa(c);
    const unsigned col_base = ((u >> LOGN) * (unsigned)(N * N) + (u & (N - 1))) * 2u + (unsigned)h * 1024u;
    uint32_t w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int t0 = 2 * m, t1 = 2 * m + 1;
        const unsigned c0 = (unsigned)((t0 >> LOGN) * 64 * N + (t0 & (N - 1)) * 2 * N);
        const unsigned c1 = (unsigned)((t1 >> LOGN) * 64 * N + (t1 & (N - 1)) * 2 * N);
        const uint32_t e0 = *reinterpret_cast<const uint16_t *>(slot + col_base + c0);
        const uint32_t e1 = *reinterpret_cast<const uint16_t *>(slot + col_base + c1);
        w[m] = e0 | (e1 << 16);
        if (PAIRWISE) __builtin_amdgcn_sched_barrier(0);              // two column reads, then their packing, pair after pair: the order the per-size kernels run fastest in
    }
    __builtin_amdgcn_wave_barrier();
    v4i lo, hi, r0, r1;
    split_planes(v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]}, v4i{(int)w[4], (int)w[5], (int)w[6], (int)w[7]}, lo, hi);
    inv_passes_with(lo, hi, k, c2r_group, r0, r1);
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

template <int LOGN>
__device__ __forceinline__ void inv_tile_in_slot(unsigned char *slot, int lane, const LaneConsts &k, const v16i &c2r)
{
    auto group = [&](int g) { return v4i{c2r[4 * g], c2r[4 * g + 1], c2r[4 * g + 2], c2r[4 * g + 3]}; };
    inv_tile_in_slot_with<LOGN, decltype(group), true>(slot, lane, k, group);
}

// Inverse transforms of the set (UNPINNED upstream; columns first, shifts 7 and 12, int16 clipping
// after each pass -- DESIGN.md section 10), contiguous batches, same block-diagonal tile idea.  The
// first contraction runs over the tile's ROW index, so each lane reads its COLUMN out of the staged
// tile (16 x ds_read_u16), exactly as the staged DCT32 inverse does.
template <int LOGN, bool INDEXED>
__device__ __forceinline__ void tr_inv_small_body(unsigned char *stage, size_t wave, const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                  size_t n_blocks, const DctOps *__restrict__ ops,
                                                  const uint32_t *__restrict__ offsets, unsigned tiles_per_wave)
{
    constexpr int N = 1 << LOGN;
    constexpr int PER = 32 / N, NSB = PER * PER;
    unsigned char *slot = stage + (threadIdx.x >> 6) * 2048;

    const int lane = threadIdx.x & 63;
    const size_t n_tiles = (n_blocks + NSB - 1) / NSB;
    size_t t = wave * tiles_per_wave;
    const size_t t_end = t + tiles_per_wave < n_tiles ? t + tiles_per_wave : n_tiles;
    if (t >= t_end) return;
    const LaneConsts k = load_consts(ops, lane);
    const v16i c2r = load_c2r(ops, lane >> 5);
    const size_t total_bytes = n_blocks * (size_t)(N * N * 2);
    for (; t < t_end; ++t) {
        size_t o0, o1;
        bool live0, live1;
        if (INDEXED) {                                                   // as in the forward kernel: chunk -> block of the offset table
            constexpr int CPB = N * N / 8;
            size_t b0 = t * NSB + (size_t)(lane / CPB), b1 = t * NSB + (size_t)((lane + 64) / CPB);
            live0 = b0 < n_blocks;
            live1 = b1 < n_blocks;
            if (!live0) b0 = n_blocks - 1;
            if (!live1) b1 = n_blocks - 1;
            o0 = ((size_t)offsets[b0] * 2) + (size_t)(lane % CPB) * 16;
            o1 = ((size_t)offsets[b1] * 2) + (size_t)((lane + 64) % CPB) * 16;
        } else {
            const size_t base = t * 2048;
            o0 = base + (size_t)lane * 16;
            o1 = o0 + 1024;
            live0 = o0 + 16 <= total_bytes;
            live1 = o1 + 16 <= total_bytes;
            if (!live0) o0 = total_bytes - 16;
            if (!live1) o1 = total_bytes - 16;
        }
        const v4i g0 = load16<true>(reinterpret_cast<const char *>(in) + o0);   // streaming hints, offset tables included (round 5: -8 % on the per-class calls over a CTU-ordered buffer, profiles/r05_result_stores.txt)
        const v4i g1 = load16<true>(reinterpret_cast<const char *>(in) + o1);
        *reinterpret_cast<v4i *>(slot + lane * 16) = g0;
        *reinterpret_cast<v4i *>(slot + 1024 + lane * 16) = g1;
        __builtin_amdgcn_wave_barrier();
        inv_tile_in_slot<LOGN>(slot, lane, k, c2r);
        __builtin_amdgcn_wave_barrier();
        const v4i s0 = *reinterpret_cast<const v4i *>(slot + lane * 16);
        const v4i s1 = *reinterpret_cast<const v4i *>(slot + 1024 + lane * 16);
        __builtin_amdgcn_wave_barrier();
        if (live0) store16m<2>(reinterpret_cast<char *>(out) + o0, s0);   // "sc1 nt" (x266_device.hpp)
        if (live1) store16m<2>(reinterpret_cast<char *>(out) + o1, s1);
    }
}

template <int LOGN>
__global__ __launch_bounds__(256) void tr_inv_small_lds_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                               size_t n_blocks, const DctOps *__restrict__ ops,
                                                               const uint32_t *__restrict__ offsets, unsigned tiles_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;       // read before the branch, as in the forward kernel
    if (LOGN == 5 || offsets) tr_inv_small_body<LOGN, true>(stage, wave, in, out, n_blocks, ops, offsets, tiles_per_wave);
    else                      tr_inv_small_body<LOGN, LOGN == 5>(stage, wave, in, out, n_blocks, ops, offsets, tiles_per_wave);
}

// ---- mixed classes, one launch (BASELINE configs[3], "batched per CTU") ------------------------------------
// A CTU's residual is a sequence of 32x32 regions ("tiles", 1024 samples), each cut into (32/N)^2 blocks of ONE
// (type, size) class, block-major.  The per-class calls above walk the buffer once per class; this kernel walks it
// once: tile t carries its class in tile_class[t] (type * 4 + log2N - 2) and sits at sample offset tile_offsets[t]
// (NULL: t * 1024).  Consecutive tiles are consecutive memory, so the access stream is that of a contiguous batch.
//
// Round 3: the operand images are no longer fetched per class from memory (class byte -> images -> first pass: two
// dependent round trips where the per-class kernels have one, 6-7 % of the launch, profiles/r03_tiles_one_launch.txt).
// Every wave copies the set's 1-D matrices in compact form (TileTab, 2 KiB, L2-resident) into LDS with its first two
// loads -- they do not depend on the class, so they travel with the tile's data -- and builds the class's images from
// there once the class byte has arrived: the block-diagonal 32x32 operand of an N-point transform is the N x N matrix
// repeated along the diagonal, so a lane's 16 operand bytes are at most 16 bytes of ONE matrix row, masked to the
// K-slots that fall into the lane's diagonal block.
// The inverse reads the table built from the TRANSPOSED matrices: pass A (vertical, columns first) M[16h + t][c] and
// pass B (horizontal) M[16h + t][kappa(c)] are both row segments there.
template <int LOGN>
__device__ __forceinline__ void inv_tile_of_class(unsigned char *slot, const unsigned char *tab, int lane, unsigned hs, unsigned vs)
{
    asm volatile("" : "+v"(lane));          // as in the forward body
    constexpr unsigned N = 1u << LOGN;
    const unsigned c = lane & 31, h = lane >> 5, kc = (unsigned)kappa((int)c);
    const unsigned mh = tile_tab_mat(0, LOGN - 2) + (LOGN == 5 ? 0u : hs * 336u), mv = tile_tab_mat(0, LOGN - 2) + (LOGN == 5 ? 0u : vs * 336u);
    const unsigned sh = tile_tab_sum(0, LOGN - 2) + (LOGN == 5 ? 0u : hs * 112u), sv = tile_tab_sum(0, LOGN - 2) + (LOGN == 5 ? 0u : vs * 112u);
    LaneConsts k;
    k.p1 = image_row_segment<LOGN>(tab + mv, c, h);
    k.p2 = image_row_segment<LOGN>(tab + mh, kc, h);
    k.tr = v4i{0, 0, 0, 0};
    k.c1 = (1 << 6) + reinterpret_cast<const int *>(tab + sv)[c & (N - 1)];
    k.c2 = 0;
    // pass-B constants per accumulator register: output column x = 16h + r, i.e. sum (16h + r) % N of the horizontal matrix
    const v4i *sums = reinterpret_cast<const v4i *>(tab + sh);
    inv_tile_in_slot_with<LOGN>(slot, lane, k, [&](int g) {
        constexpr int G = (int)N / 4;                                    // v4i groups holding the N sums
        const v4i v = LOGN == 5 ? sums[4 * h + g] : sums[g % (G < 4 ? G : 4)];
        return v4i{v[0] + (1 << 11), v[1] + (1 << 11), v[2] + (1 << 11), v[3] + (1 << 11)};
    });
}

template <bool INVERSE>
__device__ __forceinline__ void tile_of_class(unsigned char *slot, const unsigned char *tab, int lane, int cls)
{
    if (INVERSE) {
        const unsigned hs = class_h_slot(cls), vs = class_v_slot(cls);  // wave-uniform
        switch (cls & 3) {
        case 0: inv_tile_of_class<2>(slot, tab, lane, hs, vs); break;
        case 1: inv_tile_of_class<3>(slot, tab, lane, hs, vs); break;
        case 2: inv_tile_of_class<4>(slot, tab, lane, hs, vs); break;
        default: inv_tile_of_class<5>(slot, tab, lane, hs, vs); break;
        }
    } else {
        fwd_tile_of_any_class(slot, tab, lane, cls);                    // x266_transform_blocks.hpp
    }
}

// A wave takes its tiles two at a time: both tiles' data, their class bytes and (once) the table are requested with the
// wave's first instructions and parked in LDS as they arrive -- nothing is held in registers across a tile's passes.
// LDS per wave: table 2 KiB, two tile slots of 2 KiB.
template <bool INVERSE>
__device__ __forceinline__ void tr_tiles_body(unsigned char *stage, size_t wave, const int16_t *__restrict__ in, int16_t *__restrict__ out, size_t n_tiles,
                                              const uint32_t *__restrict__ tile_offsets,
                                              const uint8_t *__restrict__ tile_class, const TileTab *__restrict__ T,
                                              unsigned tiles_per_wave, unsigned lds_per_wave)
{
    unsigned char *tab = stage + (threadIdx.x >> 6) * lds_per_wave;
    unsigned char *slot0 = tab + 2048, *slot1 = tab + 4096;
    const int lane = threadIdx.x & 63;
    size_t t = wave * tiles_per_wave;
    const size_t t_end = t + tiles_per_wave < n_tiles ? t + tiles_per_wave : n_tiles;
    if (t >= t_end) return;
    t = (size_t)__builtin_amdgcn_readfirstlane((int)(t & 0xFFFFFFFFu)) | (t & ~(size_t)0xFFFFFFFFu);   // provably wave-uniform
    bool first = true;
    for (; t < t_end; t += 2) {
        const bool two = t + 1 < t_end;                                 // wave-uniform
        const int cls0 = tile_class_of(tile_class, t), cls1 = tile_class_of(tile_class, two ? t + 1 : t);
        const size_t base0 = (tile_offsets ? (size_t)tile_offsets[t] : t * 1024) * 2;
        const size_t base1 = two ? (tile_offsets ? (size_t)tile_offsets[t + 1] : (t + 1) * 1024) * 2 : base0;
        const v4i a0 = load16<true>(reinterpret_cast<const char *>(in) + base0 + lane * 16);
        const v4i a1 = load16<true>(reinterpret_cast<const char *>(in) + base0 + 1024 + lane * 16);
        if (first) {
            const char *src = reinterpret_cast<const char *>(T->b) + lane * 16;
            const v4i q0 = *reinterpret_cast<const v4i *>(src), q1 = *reinterpret_cast<const v4i *>(src + 1024);
            *reinterpret_cast<v4i *>(tab + lane * 16) = q0;
            *reinterpret_cast<v4i *>(tab + 1024 + lane * 16) = q1;
            first = false;
        }
        if (two) {
            const v4i b0 = load16<true>(reinterpret_cast<const char *>(in) + base1 + lane * 16);
            const v4i b1 = load16<true>(reinterpret_cast<const char *>(in) + base1 + 1024 + lane * 16);
            *reinterpret_cast<v4i *>(slot1 + lane * 16) = b0;
            *reinterpret_cast<v4i *>(slot1 + 1024 + lane * 16) = b1;
        }
        *reinterpret_cast<v4i *>(slot0 + lane * 16) = a0;
        *reinterpret_cast<v4i *>(slot0 + 1024 + lane * 16) = a1;
        __builtin_amdgcn_wave_barrier();
        tile_of_class<INVERSE>(slot0, tab, lane, cls0);
        __builtin_amdgcn_wave_barrier();
        {
            const v4i s0 = *reinterpret_cast<const v4i *>(slot0 + lane * 16);
            const v4i s1 = *reinterpret_cast<const v4i *>(slot0 + 1024 + lane * 16);
            char *dst = reinterpret_cast<char *>(out) + base0 + lane * 16;
            store16m<2>(dst, s0);
            store16m<2>(dst + 1024, s1);
        }
        if (two) {
            tile_of_class<INVERSE>(slot1, tab, lane, cls1);
            __builtin_amdgcn_wave_barrier();
            const v4i s0 = *reinterpret_cast<const v4i *>(slot1 + lane * 16);
            const v4i s1 = *reinterpret_cast<const v4i *>(slot1 + 1024 + lane * 16);
            char *dst = reinterpret_cast<char *>(out) + base1 + lane * 16;
            store16m<2>(dst, s0);
            store16m<2>(dst + 1024, s1);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// streaming cache hints when the tiles are the buffer in order, none behind an offset table: two complete bodies, one wave-uniform test
template <bool INVERSE>
__global__ __launch_bounds__(256) void tr_tiles_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out, size_t n_tiles,
                                                       const uint32_t *__restrict__ tile_offsets,
                                                       const uint8_t *__restrict__ tile_class, const TileTab *__restrict__ T,
                                                       unsigned tiles_per_wave, unsigned lds_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;       // read before the branch
    tr_tiles_body<INVERSE>(stage, wave, in, out, n_tiles, tile_offsets, tile_class, T, tiles_per_wave, lds_per_wave);
}

// ---- the mixed set straight from and into tiled frames, one CTU per wave ----------------------------------------------------
// A 64x64 CTU is six 32x32 regions (Y0 Y1 Y2 Y3 U V, x266_ctu_tiles.hpp), each of the class its byte names; the coefficient stream
// is 12 KiB per CTU in the tile layout of tr_tiles_kernel, so the same tile_of_class runs on the same slot contents.  Lane (c, h)
// holds row c, columns 16h .. 16h+15 of a region, and in the block-major layout of every class those 16 samples are whole
// runs: one 32-byte run (N = 32, 16), two of 16 bytes (N = 8) or four of 8 bytes (N = 4) -- exactly the fragment pieces
// fwd_tile_in_slot reads.  One wave per CTU: the 2 KiB table copy serves six regions instead of tr_tiles_kernel's two.
// Frames of any size that is a multiple of 16: lanes whose tile lies outside the frame load nothing and stand for residual 0
// (forward) or store nothing (inverse); a region wholly outside gets zero coefficients without a transform.

template <int LOGN>
__device__ __forceinline__ void get_segment_of(const unsigned char *slot, unsigned c, unsigned h, uint32_t (&d)[8])
{
    if constexpr (LOGN >= 4) {
        const unsigned char *p = slot + segment_run<LOGN>(c, h, 0);
        const v4i a = *reinterpret_cast<const v4i *>(p), b = *reinterpret_cast<const v4i *>(p + 16);
        d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3]; d[4] = b[0]; d[5] = b[1]; d[6] = b[2]; d[7] = b[3];
    } else if constexpr (LOGN == 3) {
#pragma unroll
        for (unsigned p = 0; p < 2; ++p) {
            const v4i a = *reinterpret_cast<const v4i *>(slot + segment_run<3>(c, h, p));
            d[4 * p] = a[0]; d[4 * p + 1] = a[1]; d[4 * p + 2] = a[2]; d[4 * p + 3] = a[3];
        }
    } else {
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) {
            const uint2 a = *reinterpret_cast<const uint2 *>(slot + segment_run<2>(c, h, p));
            d[2 * p] = a.x; d[2 * p + 1] = a.y;
        }
    }
}

__device__ __forceinline__ void get_segment(const unsigned char *slot, int cls, unsigned c, unsigned h, uint32_t (&d)[8])
{
    switch (cls & 3) {
    case 0: get_segment_of<2>(slot, c, h, d); break;
    case 1: get_segment_of<3>(slot, c, h, d); break;
    case 2: get_segment_of<4>(slot, c, h, d); break;
    default: get_segment_of<5>(slot, c, h, d); break;
    }
}

// forward: slot holds region q's residual (block-major for its class) -> its 2 KiB of coefficients at dst, 1 KiB-linear
__device__ __forceinline__ void fwd_region_out(unsigned char *slot, const unsigned char *tab, int lane, int cls, char *dst)
{
    tile_of_class<false>(slot, tab, lane, cls);
    __builtin_amdgcn_wave_barrier();
    const v4i s0 = *reinterpret_cast<const v4i *>(slot + lane * 16);
    const v4i s1 = *reinterpret_cast<const v4i *>(slot + 1024 + lane * 16);
    store16_sc1nt(dst, s0);
    store16_sc1nt(dst + 1024, s1);
}

__device__ __forceinline__ void zero_region_out(char *dst)
{
    const v4i z = {0, 0, 0, 0};
    store16_sc1nt(dst, z);
    store16_sc1nt(dst + 1024, z);
}

// LDS per wave: table 2 KiB + two region slots of 2 KiB; the six regions go through the slots in pairs (Y0 Y1, Y2 Y3, U V).
__global__ __launch_bounds__(256) void tr_ctu_from_tiles_kernel(const x266_ref_block_t *__restrict__ cur, const x266_ref_block_t *__restrict__ pred,
                                                                const uint8_t *__restrict__ ctu_class, int16_t *__restrict__ out,
                                                                const TileTab *__restrict__ T, int ctus_x, int tiles_x, int tiles_y,
                                                                size_t n_ctus, unsigned lds_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const int lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char *tab = stage + wave_in_wg * lds_per_wave;
    unsigned char *slot[2] = {tab + 2048, tab + 4096};
    const size_t ctu = (size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_wg;
    if (ctu >= n_ctus) return;
    const unsigned c = lane & 31, h = lane >> 5;
    const CtuPlace at = {ctu / (size_t)ctus_x, ctu % (size_t)ctus_x, tiles_x, tiles_y};
    copy_table(tab, T, lane);
    // every load of the CTU up front: four luma rows and two m_C rows per frame and lane, none outside the frame
    v4i a[4], b[4];
#pragma unroll
    for (unsigned q = 0; q < 4; ++q) {
        a[q] = b[q] = v4i{0, 0, 0, 0};
        if (ctu_luma_tile_row(at.cy, q, c) < (size_t)tiles_y && ctu_luma_tile_col(at.cx, q, h) < (size_t)tiles_x) {
            const size_t off = ctu_luma_tile(at.cy, at.cx, q, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
            a[q] = load16<true>(reinterpret_cast<const unsigned char *>(cur) + off);
            b[q] = load16<true>(reinterpret_cast<const unsigned char *>(pred) + off);
        }
    }
    v4i ca[2], cb[2];
    const bool crow = ctu_chroma_tile_row(at.cy, c) < (size_t)tiles_y;
    const size_t coff = ctu_chroma_tile(at.cy, at.cx, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
#pragma unroll
    for (unsigned j = 0; j < 2; ++j) {
        ca[j] = cb[j] = v4i{0, 0, 0, 0};
        if (crow && ctu_chroma_tile_col(at.cx, h) + j < (size_t)tiles_x) {
            ca[j] = load16<true>(reinterpret_cast<const unsigned char *>(cur) + coff + j * sizeof(x266_ref_block_t));
            cb[j] = load16<true>(reinterpret_cast<const unsigned char *>(pred) + coff + j * sizeof(x266_ref_block_t));
        }
    }
    char *dst = reinterpret_cast<char *>(out + ctu * 6144) + lane * 16;
#pragma unroll
    for (unsigned pair = 0; pair < 3; ++pair) {
        const unsigned q0 = 2 * pair, q1 = 2 * pair + 1;
        const int cls0 = tile_class_of(ctu_class, ctu * 6 + q0), cls1 = tile_class_of(ctu_class, ctu * 6 + q1);
        const bool in0 = pair == 2 || at.luma_in(q0), in1 = pair == 2 || at.luma_in(q1);   // wave-uniform; chroma is never wholly outside
        __builtin_amdgcn_wave_barrier();                                   // the previous pair has left the slots
        uint32_t d0[8], d1[8];
        if (pair < 2) {
            luma_residual16(a[q0], b[q0], d0);
            luma_residual16(a[q1], b[q1], d1);
        } else {
            chroma_residual8(ca[0], cb[0], d0, d1);
            chroma_residual8(ca[1], cb[1], d0 + 4, d1 + 4);
        }
        if (in0) put_segment(slot[0], cls0, c, h, d0);
        if (in1) put_segment(slot[1], cls1, c, h, d1);
        __builtin_amdgcn_wave_barrier();
        if (in0) fwd_region_out(slot[0], tab, lane, cls0, dst + q0 * 2048);
        else     zero_region_out(dst + q0 * 2048);
        if (in1) fwd_region_out(slot[1], tab, lane, cls1, dst + q1 * 2048);
        else     zero_region_out(dst + q1 * 2048);
    }
}

// inverse: region q's 2 KiB of coefficients (the lane's two 1 KiB-linear pieces) -> row segment d of the residual
__device__ __forceinline__ void inv_region_segment(unsigned char *slot, const unsigned char *tab, int lane, int cls, const v4i &g0, const v4i &g1,
                                                   uint32_t (&d)[8])
{
    *reinterpret_cast<v4i *>(slot + lane * 16) = g0;
    *reinterpret_cast<v4i *>(slot + 1024 + lane * 16) = g1;
    __builtin_amdgcn_wave_barrier();
    tile_of_class<true>(slot, tab, lane, cls);
    __builtin_amdgcn_wave_barrier();
    get_segment(slot, cls, (unsigned)lane & 31u, (unsigned)lane >> 5, d);
}

// Loads: the coefficients of in-frame regions (1 KiB-linear), the pred rows of in-frame lanes; stores: m_Y / m_C rows of in-frame
// lanes only.  pred and recon are not __restrict__ (recon == pred is allowed): every lane reads exactly the pred bytes it writes.
__global__ __launch_bounds__(256) void tr_ctu_to_tiles_kernel(const int16_t *__restrict__ coef, const uint8_t *__restrict__ ctu_class,
                                                              const x266_ref_block_t *pred, x266_ref_block_t *recon,
                                                              const TileTab *__restrict__ T, int ctus_x, int tiles_x, int tiles_y,
                                                              size_t n_ctus, unsigned lds_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const int lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char *tab = stage + wave_in_wg * lds_per_wave;
    unsigned char *slot[2] = {tab + 2048, tab + 4096};
    const size_t ctu = (size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_wg;
    if (ctu >= n_ctus) return;
    const unsigned c = lane & 31, h = lane >> 5;
    const CtuPlace at = {ctu / (size_t)ctus_x, ctu % (size_t)ctus_x, tiles_x, tiles_y};
    copy_table(tab, T, lane);
    const char *src = reinterpret_cast<const char *>(coef + ctu * 6144) + lane * 16;
    const unsigned char *pin = reinterpret_cast<const unsigned char *>(pred);
    unsigned char *pout = reinterpret_cast<unsigned char *>(recon);
    // every region's coefficients up front (wave-uniform: none for a region wholly outside the frame)
    v4i g[6][2];
#pragma unroll
    for (unsigned q = 0; q < 6; ++q) {
        g[q][0] = g[q][1] = v4i{0, 0, 0, 0};
        if (q >= 4 || at.luma_in(q)) {
            g[q][0] = load16<true>(src + q * 2048);
            g[q][1] = load16<true>(src + q * 2048 + 1024);
        }
    }
#pragma unroll
    for (unsigned pair = 0; pair < 3; ++pair) {
        const unsigned q0 = 2 * pair, q1 = 2 * pair + 1;
        const int cls0 = tile_class_of(ctu_class, ctu * 6 + q0), cls1 = tile_class_of(ctu_class, ctu * 6 + q1);
        const bool in0 = pair == 2 || at.luma_in(q0), in1 = pair == 2 || at.luma_in(q1);   // wave-uniform
        const v4i g0 = g[q0][0], g1 = g[q0][1], g2 = g[q1][0], g3 = g[q1][1];
        __builtin_amdgcn_wave_barrier();                                   // the previous pair has left the slots
        if (pair < 2) {
            size_t off[2];
            bool live[2];
            v4i p[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (unsigned j = 0; j < 2; ++j) {
                const unsigned q = q0 + j;
                live[j] = ctu_luma_tile_row(at.cy, q, c) < (size_t)tiles_y && ctu_luma_tile_col(at.cx, q, h) < (size_t)tiles_x;
                off[j] = ctu_luma_tile(at.cy, at.cx, q, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
                if (live[j]) p[j] = load16<true>(pin + off[j]);
            }
            uint32_t d[8];
            if (in0) {
                inv_region_segment(slot[0], tab, lane, cls0, g0, g1, d);
                if (live[0])
                    store16_sc1nt(pout + off[0], recon_luma16(p[0], v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]}, v4i{(int)d[4], (int)d[5], (int)d[6], (int)d[7]}));
            }
            if (in1) {
                inv_region_segment(slot[1], tab, lane, cls1, g2, g3, d);
                if (live[1])
                    store16_sc1nt(pout + off[1], recon_luma16(p[1], v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]}, v4i{(int)d[4], (int)d[5], (int)d[6], (int)d[7]}));
            }
        } else {
            const bool crow = ctu_chroma_tile_row(at.cy, c) < (size_t)tiles_y;
            const size_t coff = ctu_chroma_tile(at.cy, at.cx, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
            bool live[2];
            v4i p[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (unsigned j = 0; j < 2; ++j) {
                live[j] = crow && ctu_chroma_tile_col(at.cx, h) + j < (size_t)tiles_x;
                if (live[j]) p[j] = load16<true>(pin + coff + j * sizeof(x266_ref_block_t));
            }
            uint32_t du[8], dv[8];
            inv_region_segment(slot[0], tab, lane, cls0, g0, g1, du);
            inv_region_segment(slot[1], tab, lane, cls1, g2, g3, dv);
#pragma unroll
            for (unsigned j = 0; j < 2; ++j)
                if (live[j])
                    store16_sc1nt(pout + coff + j * sizeof(x266_ref_block_t),
                                  recon_chroma16(p[j], v4i{(int)du[4 * j], (int)du[4 * j + 1], (int)du[4 * j + 2], (int)du[4 * j + 3]},
                                                 v4i{(int)dv[4 * j], (int)dv[4 * j + 1], (int)dv[4 * j + 2], (int)dv[4 * j + 3]}));
        }
    }
}

}  // namespace

hipError_t launch_transform_small(int log2n, const int16_t *d_in, int16_t *d_out, size_t n_blocks, const DctOps *d_ops,
                                  const uint32_t *d_offsets, const LaunchCfg &cfg, hipStream_t stream)
{
    if (n_blocks == 0) return hipSuccess;
    const size_t per_tile = (size_t)(32 >> log2n) * (size_t)(32 >> log2n);
    const size_t tiles = (n_blocks + per_tile - 1) / per_tile;
    const unsigned tpw = units_per_wave_for(cfg, tiles);
    const size_t waves = (tiles + tpw - 1) / tpw;
    const unsigned tpb = (unsigned)cfg.wg_threads;                // same launch shape as the staged DCT32 kernel
    const size_t wpw = tpb / 64;
    unsigned wgs;
    if (hipError_t e = wave_grid(waves, wpw, &wgs)) return e;
    const size_t lds = wpw * (size_t)cfg.lds_bytes_per_wave;
    dim3 grid(wgs), block(tpb);
#define X266_TRL(L) hipLaunchKernelGGL((tr_fwd_small_lds_kernel<L>), grid, block, lds, stream, d_in, d_out, n_blocks, d_ops, d_offsets, tpw)
    if (log2n == 2) X266_TRL(2); else if (log2n == 3) X266_TRL(3); else if (log2n == 4) X266_TRL(4);
    else if (log2n == 5 && d_offsets) X266_TRL(5);                     // contiguous 32x32 batches are the DCT32 kernel's
    else return hipErrorInvalidValue;
#undef X266_TRL
    return hipGetLastError();
}

hipError_t launch_transform_small_inv(int log2n, const int16_t *d_in, int16_t *d_out, size_t n_blocks, const DctOps *d_ops,
                                      const uint32_t *d_offsets, const LaunchCfg &cfg, hipStream_t stream)
{
    if (n_blocks == 0) return hipSuccess;
    const size_t per_tile = (size_t)(32 >> log2n) * (size_t)(32 >> log2n);
    const size_t tiles = (n_blocks + per_tile - 1) / per_tile;
    const unsigned tpw = units_per_wave_for(cfg, tiles);
    const size_t waves = (tiles + tpw - 1) / tpw;
    const unsigned tpb = (unsigned)cfg.wg_threads;
    const size_t wpw = tpb / 64;
    unsigned wgs;
    if (hipError_t e = wave_grid(waves, wpw, &wgs)) return e;
    const size_t lds = wpw * (size_t)cfg.lds_bytes_per_wave;
    dim3 grid(wgs), block(tpb);
#define X266_TRI(L) hipLaunchKernelGGL((tr_inv_small_lds_kernel<L>), grid, block, lds, stream, d_in, d_out, n_blocks, d_ops, d_offsets, tpw)
    if (log2n == 2) X266_TRI(2); else if (log2n == 3) X266_TRI(3); else if (log2n == 4) X266_TRI(4);
    else if (log2n == 5 && d_offsets) X266_TRI(5);
    else return hipErrorInvalidValue;
#undef X266_TRI
    return hipGetLastError();
}

hipError_t launch_transform_tiles(bool inverse, const int16_t *d_in, int16_t *d_out, size_t n_tiles, const uint32_t *d_tile_offsets,
                                  const uint8_t *d_tile_class, const TileTab *d_tab, const LaunchCfg &cfg, hipStream_t stream)
{
    if (n_tiles == 0) return hipSuccess;
    const unsigned tpw = units_per_wave_for(cfg, n_tiles);
    const size_t waves = (n_tiles + tpw - 1) / tpw;
    const unsigned tpb = (unsigned)cfg.wg_threads;
    const size_t wpw = tpb / 64;
    unsigned wgs;
    if (hipError_t e = wave_grid(waves, wpw, &wgs)) return e;
    const unsigned per_wave = (unsigned)(cfg.lds_bytes_per_wave < 6144 ? 6144 : (cfg.lds_bytes_per_wave + 15) & ~15);   // table + two tiles, then padding
    const size_t lds = wpw * (size_t)per_wave;
    dim3 grid(wgs), block(tpb);
#define X266_TT(INV) hipLaunchKernelGGL((tr_tiles_kernel<INV>), grid, block, lds, stream, d_in, d_out, n_tiles, d_tile_offsets, d_tile_class, d_tab, tpw, per_wave)
    if (inverse) X266_TT(true); else X266_TT(false);
#undef X266_TT
    return hipGetLastError();
}

// one wave per CTU of ceil(width / 64) x ceil(height / 64); width, height multiples of 16
hipError_t launch_transform_ctu_tiles(bool inverse, const x266_ref_block_t *d_cur, const int16_t *d_coef_in, const x266_ref_block_t *d_pred,
                                      const uint8_t *d_class, int16_t *d_coef_out, x266_ref_block_t *d_recon, int width, int height,
                                      const TileTab *d_tab, const LaunchCfg &cfg, hipStream_t stream)
{
    const int ctus_x = (width + 63) / 64;
    const size_t n_ctus = (size_t)ctus_x * (size_t)((height + 63) / 64);
    if (n_ctus == 0) return hipSuccess;
    const unsigned tpb = (unsigned)cfg.wg_threads;
    const size_t wpw = tpb / 64;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_ctus, wpw, &wgs)) return e;
    const unsigned per_wave = (unsigned)(cfg.lds_bytes_per_wave < 6144 ? 6144 : (cfg.lds_bytes_per_wave + 15) & ~15);   // table + two region slots, then padding
    const size_t lds = wpw * (size_t)per_wave;
    if (inverse)
        hipLaunchKernelGGL(tr_ctu_to_tiles_kernel, dim3(wgs), dim3(tpb), lds, stream, d_coef_in, d_class, d_pred, d_recon, d_tab,
                           ctus_x, width / 16, height / 16, n_ctus, per_wave);
    else
        hipLaunchKernelGGL(tr_ctu_from_tiles_kernel, dim3(wgs), dim3(tpb), lds, stream, d_cur, d_pred, d_class, d_coef_out, d_tab,
                           ctus_x, width / 16, height / 16, n_ctus, per_wave);
    return hipGetLastError();
}

}  // namespace x266
