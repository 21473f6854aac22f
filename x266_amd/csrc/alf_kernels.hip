// alf_kernels.hip -- adaptive loop filter on tiled frames (xAlfClassifyGpu / StatsGpu / SumStatsGpu / DecideGpu / ApplyGpu of
// include/x266hip.h).  The tables, the turn G_tr, the class decision and the per-sample filter are x266_alf.hpp's, one copy.
//
// The unit of work is the CTU, as in sao_kernels.hip: one workgroup of 320 lanes, waves 0..3 its luma, wave 4 its chroma.  Phases:
//   A  the CTU's samples with their halo go into LDS rows of 18 dwords (4 bytes left of the CTU, 64 of it, 4 right of it): luma
//      rows 64 cy - 3 .. 64 cy + 66, chroma (as (U, V) pairs) rows 32 cy - 2 .. 32 cy + 33.  Coordinates are clamped per sample --
//      a dword lies wholly inside or wholly outside the plane, and one outside it is the edge sample repeated --, so LDS holds
//      r(x, y) of the header for everything the CTU reaches and no later phase knows about frame edges.
//   B  classification, statistics: luma lane = one 4x4 block (16 x 16 of them), which reads its 10 x 10 window as 10 x 3 dwords.
//      The window serves the gradient sums and, in the statistics, the twelve E of its 16 samples.
//      apply: lane = 16 consecutive bytes of one row, i.e. one 16-byte tile row of d_out (luma wave s = tile column s, lane = row;
//      chroma two rows of 8 (U, V) pairs per lane), window 7 x 6 dwords (chroma 5 x 6).
// Turned blocks.  Sample positions stay fixed and the coefficients move: position P[j] of a block turned by tr carries coefficient
// alf_turned_tap(tr, j).  Apply builds the 25 x 4 turned (coefficient, K - 1) records of the CTU's luma set in LDS once, a lane
// reads the record of each of its four blocks as six dwords.  The statistics gather E at the fixed positions into registers
// (92 words per lane, one block has one class) and turn the word index when the lane adds its block into the CTU's record.
// Statistics.  The workgroup owns the CTU's 2358 words in LDS: a luma lane adds its block's 92 sums with LDS adds, the chroma
// wave sums its 2 x 29 over its lanes by DPP and exchange and one lane writes them (an LDS add to one address from 64 lanes is a
// 64-step loop per word: 1062 us per 4K frame against 197).  Integer adds: the order does not matter.  The record goes to memory
// with plain stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_alf.hpp"
#include "x266_device.hpp"

namespace x266 {
namespace {

constexpr int kRowDwords = 18;
constexpr int kLumaHalo = 3, kChromaHalo = 2;
constexpr int kLumaRows = 64 + 2 * kLumaHalo, kChromaRows = 32 + 2 * kChromaHalo;
constexpr int kTurnedRecords = kAlfClasses * 4;                            // (class, tr) records of 6 dwords: 12 coefficients, 12 K - 1

struct Frame {
    int width, height, tiles_x, ctus_x;
};

__device__ __forceinline__ size_t luma_row_offset(const Frame &f, int x, int y)
{
    return ((size_t)(y >> 4) * (size_t)f.tiles_x + (size_t)(x >> 4)) * 512 + (size_t)((y & 15) * 16);
}
__device__ __forceinline__ size_t chroma_row_offset(const Frame &f, int x, int y)
{
    return ((size_t)(y >> 3) * (size_t)f.tiles_x + (size_t)(x >> 3)) * 512 + (size_t)(256 + (y & 7) * 16);
}

// phase A.  kChroma: a "sample" is a (U, V) pair of 2 bytes and the plane is width / 2 x height / 2
template <bool kChroma>
__device__ __forceinline__ void load_halo(const Frame &f, const uint8_t *in, uint32_t *rows, int cx, int cy, int t, int n_threads)
{
    constexpr int n_rows = kChroma ? kChromaRows : kLumaRows, per_dword = kChroma ? 2 : 4, edge = kChroma ? 32 : 64, halo = kChroma ? kChromaHalo : kLumaHalo;
    const int pw = kChroma ? f.width >> 1 : f.width, ph = kChroma ? f.height >> 1 : f.height;
    for (int i = t; i < n_rows * kRowDwords; i += n_threads) {
        const int lr = i / kRowDwords, j = i - kRowDwords * lr;
        const int x = edge * cx + per_dword * (j - 1);
        int y = edge * cy - halo + lr;
        y = y < 0 ? 0 : (y > ph - 1 ? ph - 1 : y);
        const int xc = x < 0 ? 0 : (x > pw - per_dword ? pw - per_dword : x);
        const size_t off = kChroma ? chroma_row_offset(f, xc & ~7, y) + (size_t)((xc & 7) * 2) : luma_row_offset(f, xc & ~15, y) + (size_t)(xc & 15);
        uint32_t w = *reinterpret_cast<const uint32_t *>(in + off);
        if (x < 0) w = kChroma ? (w & 0xFFFFu) * 0x10001u : (w & 0xFFu) * 0x01010101u;      // the plane's first sample, repeated
        if (x >= pw) w = kChroma ? (w >> 16) * 0x10001u : (w >> 24) * 0x01010101u;           // ... its last
        rows[i] = w;
    }
}

// byte i (a constant after unrolling) of a row of dwords
template <int N>
__device__ __forceinline__ int byte_at(const uint32_t (&w)[N], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// ---- luma, lane = 4x4 block ------------------------------------------------------------------------------------------------------
// the block's window: sample (u, v) relative to the block's first sample, u, v in -3..6, is byte u + 4 of row v + 3
struct BlockWindow {
    uint32_t w[10][3];
};

__device__ __forceinline__ void load_block_window(const uint32_t *luma, int bxl, int byl, BlockWindow &win)
{
#pragma unroll
    for (int r = 0; r < 10; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) win.w[r][k] = luma[(4 * byl + r) * kRowDwords + bxl + k];
}

__device__ __forceinline__ unsigned classify_block(const BlockWindow &win)
{
    int sv = 0, sh = 0, sd0 = 0, sd1 = 0;
#pragma unroll
    for (int v = -2; v <= 5; ++v)
#pragma unroll
        for (int u = -2; u <= 5; ++u) {
            if ((u + v) & 1) continue;                                       // the CTU's and the block's origin are even
            const int c2 = 2 * byte_at(win.w[v + 3], u + 4);
            sv += alf_abs(c2 - byte_at(win.w[v + 2], u + 4) - byte_at(win.w[v + 4], u + 4));
            sh += alf_abs(c2 - byte_at(win.w[v + 3], u + 3) - byte_at(win.w[v + 3], u + 5));
            sd0 += alf_abs(c2 - byte_at(win.w[v + 2], u + 3) - byte_at(win.w[v + 4], u + 5));
            sd1 += alf_abs(c2 - byte_at(win.w[v + 2], u + 5) - byte_at(win.w[v + 4], u + 3));
        }
    return alf_class_byte(sv, sh, sd0, sd1);
}

// The class bytes of the CTU's 256 blocks into LDS: the caller's, or computed here; a block outside the frame gets 0 and is never
// used.  d_class (may be NULL) receives the computed bytes of the blocks in the frame.  Luma lanes only.
__device__ __forceinline__ void block_classes(const Frame &f, const uint32_t *luma, int cx, int cy, int t, const uint8_t *class_in, uint8_t *class_out, uint8_t *cls)
{
    const int bxl = t & 15, byl = t >> 4, bx = 16 * cx + bxl, by = 16 * cy + byl;
    const bool inside = 4 * bx < f.width && 4 * by < f.height;
    const size_t at = (size_t)by * (size_t)(f.width >> 2) + (size_t)bx;
    unsigned b = 0;
    if (class_in) {
        if (inside) b = class_in[at];
    } else {
        BlockWindow win;
        load_block_window(luma, bxl, byl, win);
        b = classify_block(win);
        if (class_out && inside) class_out[at] = (uint8_t)b;
    }
    cls[t] = (uint8_t)b;
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// One block into the CTU's record, row by row.  acc[] is in the order of the record, but over the fixed positions P[j]; the word
// each sum belongs to follows from the block's turn.
__device__ __forceinline__ void stats_block(const uint32_t *luma, int bxl, int byl, const uint32_t (&org)[4], unsigned class_byte, int32_t *record)
{
    int acc[kAlfLumaWords] = {};
#pragma unroll 1                                                          // rolled, sample by sample: unrolled, the 92 sums spill
    for (int i = 0; i < 16; ++i) {
        const int v = i >> 2, u = i & 3;
        uint32_t w[7][2];                                                    // sample (u + dx, v + dy) is byte 4 + dx of row dy + 3
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const uint32_t *row = luma + (4 * byl + v + r) * kRowDwords + bxl;
            w[r][0] = __builtin_amdgcn_alignbyte(row[1], row[0], (unsigned)u);
            w[r][1] = __builtin_amdgcn_alignbyte(row[2], row[1], (unsigned)u);
        }
        const uint32_t o = v == 0 ? org[0] : (v == 1 ? org[1] : (v == 2 ? org[2] : org[3]));
        const int c = byte_at(w[3], 4);
        const int y = (int)((o >> (8 * u)) & 255u) - c;
        int e[kAlfLumaTaps];
#pragma unroll
        for (int j = 0; j < kAlfLumaTaps; ++j) e[j] = alf_e(c, byte_at(w[3 + kAlfLumaDy[j]], 4 + kAlfLumaDx[j]), byte_at(w[3 - kAlfLumaDy[j]], 4 - kAlfLumaDx[j]));
        acc[0] += 1;
        acc[1] += __mul24(y, y);
#pragma unroll
        for (int j = 0; j < kAlfLumaTaps; ++j) {
            acc[2 + j] += __mul24(e[j], y);
#pragma unroll
            for (int k = j; k < kAlfLumaTaps; ++k) acc[alf_a_word(kAlfLumaTaps, j, k)] += __mul24(e[j], e[k]);
        }
    }
    int32_t *rec = record + alf_class_of(class_byte) * kAlfLumaWords;
    const unsigned sh = 4u * (unsigned)alf_turn_of(class_byte);
    int turned[kAlfLumaTaps];
#pragma unroll
    for (int j = 0; j < kAlfLumaTaps; ++j) turned[j] = (int)((alf_turned_taps(j) >> sh) & 15u);
    atomicAdd(&rec[0], acc[0]);
    atomicAdd(&rec[1], acc[1]);
#pragma unroll
    for (int j = 0; j < kAlfLumaTaps; ++j) {
        atomicAdd(&rec[2 + turned[j]], acc[2 + j]);
#pragma unroll
        for (int k = j; k < kAlfLumaTaps; ++k) {
            const int a = turned[j] < turned[k] ? turned[j] : turned[k], b = turned[j] < turned[k] ? turned[k] : turned[j];
            atomicAdd(&rec[alf_a_word(kAlfLumaTaps, a, b)], acc[alf_a_word(kAlfLumaTaps, j, k)]);
        }
    }
}

// the chroma window of a lane's 8 (U, V) pairs: pair i + dx of row dy is bytes 4 + 2 (i + dx) + {0, 1} of row dy + 2
struct ChromaWindow {
    uint32_t w[5][6];
};

__device__ __forceinline__ void load_chroma_window(const uint32_t *chroma, int s, int r, ChromaWindow &win)
{
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) win.w[k][i] = chroma[(r + k) * kRowDwords + 4 * s + i];
}

// 8 pairs into the lane's U and V sums, acc[m] in the order of the record
__device__ __forceinline__ void stats_chroma(const ChromaWindow &win, const v4i &org, int (&acc)[2][kAlfChromaWords])
{
    const uint32_t o[4] = {(uint32_t)org.x, (uint32_t)org.y, (uint32_t)org.z, (uint32_t)org.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = i & 1, c = byte_at(win.w[2], 4 + i), y = byte_at(o, i) - c;
        int e[kAlfChromaTaps];
#pragma unroll
        for (int j = 0; j < kAlfChromaTaps; ++j)
            e[j] = alf_e(c, byte_at(win.w[2 + kAlfChromaDy[j]], 4 + i + 2 * kAlfChromaDx[j]), byte_at(win.w[2 - kAlfChromaDy[j]], 4 + i - 2 * kAlfChromaDx[j]));
        acc[m][0] += 1;
        acc[m][1] += __mul24(y, y);
#pragma unroll
        for (int j = 0; j < kAlfChromaTaps; ++j) {
            acc[m][2 + j] += __mul24(e[j], y);
#pragma unroll
            for (int k = j; k < kAlfChromaTaps; ++k) acc[m][alf_a_word(kAlfChromaTaps, j, k)] += __mul24(e[j], e[k]);
        }
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
// a dword of a read-only table as a wave-uniform value (s_load through a constant-address-space pointer, as uniform_byte)
__device__ __forceinline__ uint32_t uniform_dword(const void *p, int i)
{
    typedef const __attribute__((address_space(4))) uint32_t *const_dword_ptr;
    const const_dword_ptr w = (const_dword_ptr) reinterpret_cast<uintptr_t>(p);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)w[i]);
}

// the CTU's luma set as 100 turned records; luma lanes
__device__ __forceinline__ void build_turned_records(const x266_alf_luma_t *set, uint32_t *turned, int t)
{
    uint8_t *out = reinterpret_cast<uint8_t *>(turned);
    for (int e = t; e < kTurnedRecords * kAlfLumaTaps; e += 256) {
        const int rec = e / kAlfLumaTaps, j = e - rec * kAlfLumaTaps, cls = rec >> 2, tr = rec & 3;
        int i = 0;
#pragma unroll
        for (int q = 0; q < kAlfLumaTaps; ++q) i = j == q ? (int)((alf_turned_taps(q) >> (4 * tr)) & 15u) : i;
        out[rec * 24 + j] = (uint8_t)set->coef[cls][i];
        out[rec * 24 + 12 + j] = (uint8_t)alf_clip_minus_1(set->clip[cls][i]);
    }
}

// one tile row of luma: 16 samples from the lane's 7 x 6 dword window (sample i is byte 4 + i of row 3)
__device__ __forceinline__ void filter_luma_row(const uint32_t *luma, const uint32_t *turned, uint32_t class4, int s, int r, uint32_t (&out)[4])
{
    uint32_t win[7][6];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) win[k][i] = luma[(r + k) * kRowDwords + 4 * s + i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned b = (class4 >> (8 * q)) & 255u;
        const uint32_t *rec = turned + (alf_class_of(b) * 4 + alf_turn_of(b)) * 6;
        uint32_t cw[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) cw[i] = rec[i];
        uint32_t packed = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 4 * q + u, c = byte_at(win[3], 4 + i);
            int sum = 0;
#pragma unroll
            for (int j = 0; j < kAlfLumaTaps; ++j) {
                const int coef = (int)(int8_t)byte_at(cw, j), k = byte_at(cw, 12 + j) + 1;
                sum += alf_tap(coef, k, c, byte_at(win[3 + kAlfLumaDy[j]], 4 + i + kAlfLumaDx[j]), byte_at(win[3 - kAlfLumaDy[j]], 4 + i - kAlfLumaDx[j]));
            }
            packed |= (uint32_t)alf_round(c, sum) << (8 * u);
        }
        out[q] = packed;
    }
}

// the bytes kPhase, kPhase + 2, ... (U or V) of a chroma row under one alternative, given as four uniform dwords
template <int kPhase>
__device__ __forceinline__ void filter_chroma_row(const ChromaWindow &win, const uint32_t (&alt)[4], uint32_t (&out)[4])
{
#pragma unroll
    for (int i = kPhase; i < 16; i += 2) {
        const int c = byte_at(win.w[2], 4 + i);
        int sum = 0;
#pragma unroll
        for (int j = 0; j < kAlfChromaTaps; ++j) {
            const int coef = (int)(int8_t)byte_at(alt, j), k = (int)alf_clip_minus_1((unsigned)byte_at(alt, 6 + j)) + 1;
            sum += alf_tap(coef, k, c, byte_at(win.w[2 + kAlfChromaDy[j]], 4 + i + 2 * kAlfChromaDx[j]), byte_at(win.w[2 - kAlfChromaDy[j]], 4 + i - 2 * kAlfChromaDx[j]));
        }
        out[i >> 2] = (out[i >> 2] & ~(255u << (8 * (i & 3)))) | (uint32_t)alf_round(c, sum) << (8 * (i & 3));
    }
}

// ---- kernels: blockIdx.x walks the CTUs in raster order ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void alf_classify_kernel(const uint8_t *dec, Frame f, uint8_t *class_out)
{
    __shared__ uint32_t luma[kLumaRows * kRowDwords];
    __shared__ uint8_t cls[256];
    const int t = (int)threadIdx.x, cy = (int)(blockIdx.x / (unsigned)f.ctus_x), cx = (int)(blockIdx.x - (unsigned)cy * (unsigned)f.ctus_x);
    load_halo<false>(f, dec, luma, cx, cy, t, 256);
    __syncthreads();
    block_classes(f, luma, cx, cy, t, nullptr, class_out, cls);
}

__global__ __launch_bounds__(320) void alf_stats_kernel(const uint8_t *org, const uint8_t *dec, Frame f, const uint8_t *class_in, int32_t *stats)
{
    __shared__ uint32_t luma[kLumaRows * kRowDwords];
    __shared__ uint32_t chroma[kChromaRows * kRowDwords];
    __shared__ int32_t record[kAlfCtuWords];
    const int t = (int)threadIdx.x, cy = (int)(blockIdx.x / (unsigned)f.ctus_x), cx = (int)(blockIdx.x - (unsigned)cy * (unsigned)f.ctus_x);
    const bool is_luma = t < 256;                                         // uniform per wave
    for (int i = t; i < kAlfCtuWords; i += 320) record[i] = 0;
    if (is_luma) load_halo<false>(f, dec, luma, cx, cy, t, 256);
    else         load_halo<true>(f, dec, chroma, cx, cy, t - 256, 64);
    __syncthreads();
    if (is_luma) {
        const int bxl = t & 15, byl = t >> 4, x = 64 * cx + 4 * bxl, y = 64 * cy + 4 * byl;
        if (x < f.width && y < f.height) {
            unsigned b;
            if (class_in) {
                b = class_in[(size_t)(y >> 2) * (size_t)(f.width >> 2) + (size_t)(x >> 2)];
            } else {
                BlockWindow win;
                load_block_window(luma, bxl, byl, win);
                b = classify_block(win);
            }
            uint32_t o[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = *reinterpret_cast<const uint32_t *>(org + luma_row_offset(f, x & ~15, y + v) + (size_t)(x & 15));
            stats_block(luma, bxl, byl, o, b, record);
        }
    } else {
        int acc[2][kAlfChromaWords] = {};
#pragma unroll 1
        for (int it = 0; it < 2; ++it) {
            const int q = t - 256 + 64 * it, s = q >> 5, r = q & 31, x = 32 * cx + 8 * s, y = 32 * cy + r;
            if (x < (f.width >> 1) && y < (f.height >> 1)) {
                ChromaWindow win;
                load_chroma_window(chroma, s, r, win);
                stats_chroma(win, load16<false>(org + chroma_row_offset(f, x, y)), acc);
            }
        }
        // the wave's sums: over rows of 16 lanes by DPP, over the four rows by two exchanges; no other wave touches these words
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < kAlfChromaWords; ++i) {
                int v = (int)sum_over_row16((uint32_t)acc[m][i]);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (t == 256) record[kAlfClasses * kAlfLumaWords + m * kAlfChromaWords + i] = v;
            }
    }
    __syncthreads();
    for (int i = t; i < kAlfCtuWords; i += 320) stats[(size_t)blockIdx.x * kAlfCtuWords + (size_t)i] = record[i];
}

// 32 consecutive words of the record x 32 slices of the CTUs per workgroup; the slices meet in LDS
__global__ __launch_bounds__(1024) void alf_sum_stats_kernel(const int32_t *stats, unsigned n_ctu, const uint8_t *mask, int64_t *total)
{
    __shared__ int64_t part[32][33];
    const int lane = (int)(threadIdx.x & 31), slice = (int)(threadIdx.x >> 5), word = (int)blockIdx.x * 32 + lane;
    int64_t sum = 0;
    if (word < kAlfCtuWords)
        for (unsigned c = (unsigned)slice; c < n_ctu; c += 32)
            if (!mask || mask[c]) sum += (int64_t)stats[(size_t)c * kAlfCtuWords + (size_t)word];
    part[slice][lane] = sum;
    __syncthreads();
    if (slice == 0 && word < kAlfCtuWords) {
        int64_t all = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) all += part[i][lane];
        total[word] = all;
    }
}

// the cost of one class record (n taps) under coefficients c: sum c_i^2 A_ii + 2 sum_{i<j} c_i c_j A_ij - 256 sum c_i b_i
template <int N>
__device__ __forceinline__ int64_t record_cost(const int32_t *rec, const int8_t *coef)
{
    int c[N];
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = coef[i];
    int64_t cost = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        cost -= (int64_t)(256 * c[i]) * (int64_t)rec[2 + i];
#pragma unroll
        for (int j = i; j < N; ++j) cost += (int64_t)((i == j ? 1 : 2) * c[i] * c[j]) * (int64_t)rec[alf_a_word(N, i, j)];
    }
    return cost;
}

// four CTUs per workgroup, one per wave (a wave past the last CTU only keeps the barrier company): lanes 0..24 the luma classes,
// lanes 32, 33 U and V
__global__ __launch_bounds__(256) void alf_decide_kernel(const int32_t *stats, unsigned n_ctu, const x266_alf_luma_t *luma, int n_luma, const x266_alf_chroma_t *chroma,
                                                         int n_chroma, int lambda_q4, uint8_t *ctrl)
{
    __shared__ int32_t records[4][kAlfCtuWords];
    const int lane = (int)(threadIdx.x & 63);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ctu = blockIdx.x * 4 + wave;
    const bool active = ctu < n_ctu;                                        // uniform per wave
    int32_t *rec = records[wave];
    if (active)
        for (int i = lane; i < kAlfCtuWords; i += 64) rec[i] = stats[(size_t)ctu * kAlfCtuWords + (size_t)i];
    __syncthreads();
    if (!active) return;
    const bool is_class = lane < kAlfClasses, is_chroma = lane == 32 || lane == 33;
    const int32_t *mine = is_class ? rec + lane * kAlfLumaWords : rec + kAlfClasses * kAlfLumaWords + (lane & 1) * kAlfChromaWords;
    const int64_t luma_count = wave_sum(is_class ? (int64_t)mine[0] : 0);
    const int64_t rate_luma = ((int64_t)lambda_q4 << 10) * alf_ceil_log2(n_luma), rate_chroma = ((int64_t)lambda_q4 << 10) * alf_ceil_log2(n_chroma);
    int64_t best_luma = 0, best_chroma = 0;
    int pick_luma = 0, pick_chroma = 0;
    for (int s = 0; s < kAlfMaxSets; ++s) {
        int64_t cost = 0;
        if (is_class && s < n_luma) cost = record_cost<kAlfLumaTaps>(mine, luma[s].coef[lane]);
        const int64_t j_luma = wave_sum(is_class ? cost : 0) + rate_luma;
        if (s < n_luma && j_luma < best_luma) { best_luma = j_luma; pick_luma = s + 1; }
        if (is_chroma && s < n_chroma) {
            const int64_t j = record_cost<kAlfChromaTaps>(mine, chroma[s].coef) + rate_chroma;
            if (j < best_chroma) { best_chroma = j; pick_chroma = s + 1; }
        }
    }
    if (lane == 0) ctrl[(size_t)ctu * 3] = (uint8_t)(luma_count != 0 ? pick_luma : 0);
    if (is_chroma) ctrl[(size_t)ctu * 3 + 1 + (size_t)(lane & 1)] = (uint8_t)(mine[0] != 0 ? pick_chroma : 0);
}

__global__ __launch_bounds__(320) void alf_apply_kernel(const uint8_t *in, uint8_t *out, Frame f, const uint8_t *class_in, const x266_alf_luma_t *luma_sets, int n_luma,
                                                        const x266_alf_chroma_t *chroma_alts, int n_chroma, const uint8_t *ctrl)
{
    __shared__ uint32_t luma[kLumaRows * kRowDwords];
    __shared__ uint32_t chroma[kChromaRows * kRowDwords];
    __shared__ uint32_t turned[kTurnedRecords * 6];
    __shared__ __attribute__((aligned(4))) uint8_t cls[256];
    const int t = (int)threadIdx.x, cy = (int)(blockIdx.x / (unsigned)f.ctus_x), cx = (int)(blockIdx.x - (unsigned)cy * (unsigned)f.ctus_x);
    const bool is_luma = t < 256;                                         // uniform per wave
    const int pick_y = (int)uniform_byte(ctrl, (size_t)blockIdx.x * 3);
    const bool filter_y = pick_y >= 1 && pick_y <= n_luma;                // uniform over the workgroup
    if (is_luma) {
        load_halo<false>(f, in, luma, cx, cy, t, 256);
        if (filter_y) build_turned_records(luma_sets + (pick_y - 1), turned, t);
    } else {
        load_halo<true>(f, in, chroma, cx, cy, t - 256, 64);
    }
    __syncthreads();
    if (is_luma && filter_y) block_classes(f, luma, cx, cy, t, class_in, nullptr, cls);
    __syncthreads();
    if (is_luma) {
        const int s = t >> 6, r = t & 63, x = 64 * cx + 16 * s, y = 64 * cy + r;
        if (x < f.width && y < f.height) {
            uint32_t c[4];
            if (filter_y) {
                filter_luma_row(luma, turned, reinterpret_cast<const uint32_t *>(cls)[(r >> 2) * 4 + s], s, r, c);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = luma[(r + kLumaHalo) * kRowDwords + 1 + 4 * s + i];
            }
            store16<true>(out + luma_row_offset(f, x, y), v4i{(int)c[0], (int)c[1], (int)c[2], (int)c[3]});
        }
    } else {
        const int pick_u = (int)uniform_byte(ctrl, (size_t)blockIdx.x * 3 + 1), pick_v = (int)uniform_byte(ctrl, (size_t)blockIdx.x * 3 + 2);
        const bool filter_u = pick_u >= 1 && pick_u <= n_chroma, filter_v = pick_v >= 1 && pick_v <= n_chroma;
        uint32_t alt_u[4] = {}, alt_v[4] = {};
        if (filter_u)
#pragma unroll
            for (int i = 0; i < 4; ++i) alt_u[i] = uniform_dword(chroma_alts + (pick_u - 1), i);
        if (filter_v)
#pragma unroll
            for (int i = 0; i < 4; ++i) alt_v[i] = uniform_dword(chroma_alts + (pick_v - 1), i);
#pragma unroll 1
        for (int it = 0; it < 2; ++it) {
            const int q = t - 256 + 64 * it, s = q >> 5, r = q & 31, x = 32 * cx + 8 * s, y = 32 * cy + r;
            if (x < (f.width >> 1) && y < (f.height >> 1)) {
                ChromaWindow win;
                load_chroma_window(chroma, s, r, win);
                uint32_t c[4] = {win.w[2][1], win.w[2][2], win.w[2][3], win.w[2][4]};
                if (filter_u) filter_chroma_row<0>(win, alt_u, c);
                if (filter_v) filter_chroma_row<1>(win, alt_v, c);
                store16<true>(out + chroma_row_offset(f, x, y), v4i{(int)c[0], (int)c[1], (int)c[2], (int)c[3]});
            }
        }
    }
}

Frame frame_of(int width, int height)
{
    Frame f;
    f.width = width;
    f.height = height;
    f.tiles_x = width / 16;
    f.ctus_x = (width + 63) / 64;
    return f;
}

// the CTUs of a frame, or 0 if the count does not fit a grid
unsigned ctus_of(const Frame &f)
{
    const size_t n = (size_t)f.ctus_x * (size_t)((f.height + 63) / 64);
    return n > 0x7FFFFFFFull ? 0u : (unsigned)n;
}

}  // namespace

hipError_t launch_alf_classify(const x266_ref_block_t *d_dec, int width, int height, uint8_t *d_class, hipStream_t stream)
{
    const Frame f = frame_of(width, height);
    const unsigned n_ctu = ctus_of(f);
    if (!n_ctu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alf_classify_kernel, dim3(n_ctu), dim3(256), 0, stream, reinterpret_cast<const uint8_t *>(d_dec), f, d_class);
    return hipGetLastError();
}

hipError_t launch_alf_stats(const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, const uint8_t *d_class, int32_t *d_stats,
                            hipStream_t stream)
{
    const Frame f = frame_of(width, height);
    const unsigned n_ctu = ctus_of(f);
    if (!n_ctu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alf_stats_kernel, dim3(n_ctu), dim3(320), 0, stream, reinterpret_cast<const uint8_t *>(d_org), reinterpret_cast<const uint8_t *>(d_dec), f,
                       d_class, d_stats);
    return hipGetLastError();
}

hipError_t launch_alf_sum_stats(const int32_t *d_stats, size_t n_ctu, const uint8_t *d_mask, int64_t *d_total, hipStream_t stream)
{
    if (n_ctu > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alf_sum_stats_kernel, dim3((kAlfCtuWords + 31) / 32), dim3(1024), 0, stream, d_stats, (unsigned)n_ctu, d_mask, d_total);
    return hipGetLastError();
}

hipError_t launch_alf_decide(const int32_t *d_stats, size_t n_ctu, const x266_alf_luma_t *d_luma, int n_luma, const x266_alf_chroma_t *d_chroma, int n_chroma,
                             int lambda_q4, uint8_t *d_ctrl, hipStream_t stream)
{
    if (n_ctu > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alf_decide_kernel, dim3((unsigned)((n_ctu + 3) / 4)), dim3(256), 0, stream, d_stats, (unsigned)n_ctu, d_luma, n_luma, d_chroma, n_chroma,
                       lambda_q4, d_ctrl);
    return hipGetLastError();
}

hipError_t launch_alf_apply(const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const uint8_t *d_class, const x266_alf_luma_t *d_luma,
                            int n_luma, const x266_alf_chroma_t *d_chroma, int n_chroma, const uint8_t *d_ctrl, hipStream_t stream)
{
    const Frame f = frame_of(width, height);
    const unsigned n_ctu = ctus_of(f);
    if (!n_ctu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alf_apply_kernel, dim3(n_ctu), dim3(320), 0, stream, reinterpret_cast<const uint8_t *>(d_in), reinterpret_cast<uint8_t *>(d_out), f, d_class,
                       d_luma, n_luma, d_chroma, n_chroma, d_ctrl);
    return hipGetLastError();
}

}  // namespace x266
