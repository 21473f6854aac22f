// sao_kernels.hip -- sample adaptive offset on tiled frames (xSaoStatsGpu / DecideGpu / SearchGpu / ApplyGpu of include/x266hip.h).
// The per-sample arithmetic and the per-bin offset search are x266_sao.hpp's, one copy for the four kernels.
//
// The unit of work is the unmoved CTU: one workgroup of 320 lanes, waves 0..3 its luma (wave s = the 16-sample tile column s, lane =
// row), wave 4 its chroma (two tile rows of 8 (U, V) pairs per lane), the role fixed per wave as in deblock_kernel.  Phases:
//   A  the CTU's `dec` samples with a one-sample halo go into LDS rows as dwords: luma x = 64 cx - 4 .. 64 cx + 67 on rows 64 cy - 1 ..
//      64 cy + 64, chroma the same in pairs.  Coordinates are clamped into the plane, so every load is in bounds; what a clamped
//      position holds is never used, because the lane that would use it knows from its coordinates that the neighbour lies outside
//      the plane and gives the sample category 0 for that class.
//   B  a lane takes 16 consecutive bytes of one row -- one 16-byte tile row of `org` (statistics) or of `out` (apply) -- and reads its
//      own row segment and the neighbour segments from LDS as dwords shifted to the neighbour's byte offset: no byte loads, and the
//      EO class only changes an LDS offset that is uniform over the workgroup.
// Statistics.  EO bins: a lane adds (1 << 16) + (org - dec) into one register per bin (at most 16 samples per lane and bin: the count
// sits in the high half, the signed sum in the low half), unpacks, sums over its row of 16 lanes by DPP and one lane per row adds into
// the workgroup's LDS bins.  Bands are data-dependent: a lane merges its run of equal bands in a register and adds it to the LDS bins
// when the band changes -- neighbouring samples mostly share a band, so this is a few LDS adds per lane instead of 16, and it needs
// neither 32 registers per lane nor per-wave copies of the bins.  All adds are integer adds: the result does not depend on order.
// Decision: one wave per CTU, a lane per bin (x266_sao.hpp: sao_bin_search), class sums and the 29 window sums through LDS, the
// least window by a wave minimum over (cost, position) keys (wave_min, x266_lanes.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_sao.hpp"

namespace x266 {
namespace {

constexpr int kRowDwords = 18;              // LDS row: 4 bytes left of the CTU, 64 bytes of it, 4 bytes right of it
constexpr int kRowBytes = 4 * kRowDwords;
constexpr int kLumaRows = 66, kChromaRows = 34;
constexpr int kCtuWords = 3 * kSaoBins * 2; // 288 dwords of bins per CTU

struct Frame {
    int width, height, tiles_x, ctus_x;
};

struct DecideScratch {
    int32_t cost[3][kSaoBins];
    int32_t off[3][kSaoBins];
};

// byte offset in a frame of the 16-byte tile row that holds luma sample (x, y), x a multiple of 16
__device__ __forceinline__ size_t luma_row_offset(const Frame &f, int x, int y)
{
    return ((size_t)(y >> 4) * (size_t)f.tiles_x + (size_t)(x >> 4)) * 512 + (size_t)((y & 15) * 16);
}
// ... of the m_C row that holds the (U, V) pair of chroma sample (x, y), x a multiple of 8
__device__ __forceinline__ size_t chroma_row_offset(const Frame &f, int x, int y)
{
    return ((size_t)(y >> 3) * (size_t)f.tiles_x + (size_t)(x >> 3)) * 512 + (size_t)(256 + (y & 7) * 16);
}

// phase A.  kChroma: a "sample" is a (U, V) pair of 2 bytes and the plane is width / 2 x height / 2
template <bool kChroma>
__device__ __forceinline__ void load_halo(const Frame &f, const uint8_t *in, uint32_t *rows, int cx, int cy, int t, int n_threads)
{
    constexpr int n_rows = kChroma ? kChromaRows : kLumaRows, per_dword = kChroma ? 2 : 4, edge = kChroma ? 32 : 64;
    const int pw = kChroma ? f.width >> 1 : f.width, ph = kChroma ? f.height >> 1 : f.height;
    for (int i = t; i < n_rows * kRowDwords; i += n_threads) {
        const int lr = i / kRowDwords, j = i - kRowDwords * lr;
        int x = edge * cx + per_dword * (j - 1), y = edge * cy - 1 + lr;
        x = x < 0 ? 0 : (x > pw - per_dword ? pw - per_dword : x);
        y = y < 0 ? 0 : (y > ph - 1 ? ph - 1 : y);
        const size_t off = kChroma ? chroma_row_offset(f, x & ~7, y) + (size_t)((x & 7) * 2) : luma_row_offset(f, x & ~15, y) + (size_t)(x & 15);
        rows[i] = *reinterpret_cast<const uint32_t *>(in + off);
    }
}

// 16 bytes from byte `d` (any sign, any alignment) after dword `base` of the LDS rows
__device__ __forceinline__ void seg16(const uint32_t *rows, int base, int d, uint32_t (&out)[4])
{
    const uint32_t *p = rows + base + (d >> 2);
    const unsigned sh = 8u * (unsigned)(d & 3);
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = p[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | (uint64_t)w[i]) >> sh);
}

__device__ __forceinline__ int byte_of(const uint32_t (&w)[4], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// byte distance from a sample to neighbour a of EO class k (b is at minus that); kStep = bytes per sample in a row (2 for (U, V) pairs)
template <int kStep>
__device__ __forceinline__ int neighbour_a(int k)
{
    return k == 0 ? -kStep : (k == 1 ? -kRowBytes : (k == 2 ? -kRowBytes - kStep : -kRowBytes + kStep));
}

// what a lane knows about its segment: whether it lies in the frame, and which of its neighbours do not
struct Segment {
    int base;                                // dword of the segment's first byte in the LDS rows
    bool valid, left, right, vert;           // in the frame; first sample on the plane's left edge; last on its right; row on the top or bottom
};

__device__ __forceinline__ Segment make_segment(int s, int r, int x, int y, int pw, int ph, int samples)
{
    Segment g;
    g.base = (r + 1) * kRowDwords + 1 + 4 * s;
    g.valid = x < pw && y < ph;
    g.left = x == 0;
    g.right = x + samples == pw;
    g.vert = y == 0 || y == ph - 1;
    return g;
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------
struct BandRun {
    int band;
    uint32_t acc;                            // (count << 16) + sum of the run
};

__device__ __forceinline__ void unpack(uint32_t acc, int &count, int &sum)
{
    sum = (int)(int16_t)(acc & 0xFFFFu);
    count = (int)((acc - (uint32_t)sum) >> 16);
}

__device__ __forceinline__ void flush_run(const BandRun &run, int32_t *bins)
{
    if (run.acc) {
        int count, sum;
        unpack(run.acc, count, sum);
        atomicAdd(&bins[(16 + run.band) * 2], count);
        atomicAdd(&bins[(16 + run.band) * 2 + 1], sum);
    }
}

// one segment into the lane's EO registers and band runs; bins: the LDS bins of the segment's first component (the next one's follow)
template <int kStep>
__device__ __forceinline__ void stats_segment(const uint32_t *rows, const Segment &g, const v4i &org, uint32_t (&acc)[kStep][16], BandRun (&run)[kStep],
                                              int32_t *bins)
{
    uint32_t c[4];
    seg16(rows, g.base, 0, c);
    const uint32_t o[4] = {(uint32_t)org.x, (uint32_t)org.y, (uint32_t)org.z, (uint32_t)org.w};
    // class by class, so that only one pair of neighbour segments is live at a time
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t a[4], b[4];
        seg16(rows, g.base, neighbour_a<kStep>(k), a);
        seg16(rows, g.base, -neighbour_a<kStep>(k), b);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = i % kStep, ci = byte_of(c, i);
            const uint32_t packed = g.valid ? (1u << 16) + (uint32_t)(byte_of(o, i) - ci) : 0u;
            const bool hm = (g.left && i < kStep) || (g.right && i >= 16 - kStep);
            const bool outside = k == 0 ? hm : (k == 1 ? g.vert : (hm || g.vert));
            const int cat = outside ? 0 : sao_category(ci, byte_of(a, i), byte_of(b, i));
#pragma unroll
            for (int q = 1; q <= 4; ++q) acc[m][4 * k + q - 1] += cat == q ? packed : 0u;
        }
    }
    if (g.valid) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = i % kStep, ci = byte_of(c, i), band = sao_band(ci);
            if (band != run[m].band) {
                flush_run(run[m], bins + m * kSaoBins * 2);
                run[m].band = band;
                run[m].acc = 0;
            }
            run[m].acc += (1u << 16) + (uint32_t)(byte_of(o, i) - ci);
        }
    }
}

// the lane's registers into the LDS bins; every lane of the wave comes here
template <int kStep>
__device__ __forceinline__ void stats_reduce(const uint32_t (&acc)[kStep][16], const BandRun (&run)[kStep], int32_t *bins, int lane)
{
#pragma unroll
    for (int m = 0; m < kStep; ++m) {
        flush_run(run[m], bins + m * kSaoBins * 2);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            int count, sum;
            unpack(acc[m][e], count, sum);
            count = (int)sum_over_row16((uint32_t)count);
            sum = (int)sum_over_row16((uint32_t)sum);
            if ((lane & 15) == 0 && count) {
                atomicAdd(&bins[(m * kSaoBins + e) * 2], count);
                atomicAdd(&bins[(m * kSaoBins + e) * 2 + 1], sum);
            }
        }
    }
}

// ---- decision: one wave, lane = bin.  Every thread of the workgroup calls this (it holds barriers); `active` is uniform per wave ----
__device__ __forceinline__ void sao_decide(const int32_t *bins, DecideScratch &scr, int lambda_q4, x266_sao_t *out, int lane, bool active)
{
    if (active && lane < kSaoBins) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            int cost;
            scr.off[m][lane] = sao_bin_search(lane, bins[(m * kSaoBins + lane) * 2], bins[(m * kSaoBins + lane) * 2 + 1], lambda_q4, cost);
            scr.cost[m][lane] = cost;
        }
    }
    __syncthreads();
    if (!active) return;
    int eo[3][4], bo[3], pos[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int k = 0; k < 4; ++k) eo[m][k] = scr.cost[m][4 * k] + scr.cost[m][4 * k + 1] + scr.cost[m][4 * k + 2] + scr.cost[m][4 * k + 3];
        const int p = lane < 29 ? lane : 28;
        const int window = scr.cost[m][16 + p] + scr.cost[m][17 + p] + scr.cost[m][18 + p] + scr.cost[m][19 + p];
        const int64_t key = wave_min(lane < 29 ? (int64_t)window * 32 + p : INT64_MAX);      // least cost, then least position
        pos[m] = (int)(key & 31);
        bo[m] = (int)((key - pos[m]) / 32);
    }
    // candidates in the header's order; a later one must be strictly cheaper
    int type_y = 0, arg_y = 0, best = lambda_q4;
    int type_c = 0, class_c = 0, best_c = lambda_q4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int jy = 4 * lambda_q4 + eo[0][k], jc = 4 * lambda_q4 + eo[1][k] + eo[2][k];
        if (jy < best) { best = jy; type_y = 2; arg_y = k; }
        if (jc < best_c) { best_c = jc; type_c = 2; class_c = k; }
    }
    if (7 * lambda_q4 + bo[0] < best) { type_y = 1; arg_y = pos[0]; }
    if (12 * lambda_q4 + bo[1] + bo[2] < best_c) type_c = 1;
    if (lane < 3) {
        const int type = lane == 0 ? type_y : type_c;
        const int arg = lane == 0 ? arg_y : (type_c == 2 ? class_c : (type_c == 1 ? (lane == 1 ? pos[1] : pos[2]) : 0));
        const int first = type == 2 ? 4 * arg : 16 + arg;
        uint64_t rec = (uint64_t)type | (uint64_t)arg << 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) rec |= (uint64_t)(type ? (uint32_t)scr.off[lane][first + i] & 255u : 0u) << (16 + 8 * i);
        *reinterpret_cast<uint64_t *>(out + lane) = rec;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
// a CTU component's record as a wave-uniform value (s_load through a constant-address-space pointer, as uniform_byte)
__device__ __forceinline__ uint64_t uniform_record(const x266_sao_t *p)
{
    typedef const __attribute__((address_space(4))) uint32_t *const_dword_ptr;
    const const_dword_ptr w = (const_dword_ptr) reinterpret_cast<uintptr_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[0]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[1]);
    return (uint64_t)hi << 32 | lo;
}

// the bytes kPhase, kPhase + kStep, ... of a segment under one record; type and class are uniform, so no lane diverges here
template <int kStep, int kPhase>
__device__ __forceinline__ void apply_component(const uint32_t *rows, const Segment &g, uint64_t rec, uint32_t (&c)[4])
{
    const unsigned type = (unsigned)(rec & 255u), arg = (unsigned)(rec >> 8) & 255u;
    const uint32_t offs = (uint32_t)(rec >> 16);
    if (type == 2) {
        const int k = (int)(arg & 3u), da = neighbour_a<kStep>(k);
        const bool use_h = k != 1, use_v = k != 0;
        uint32_t a[4], b[4];
        seg16(rows, g.base, da, a);
        seg16(rows, g.base, -da, b);
        const uint32_t lo = (offs & 0xFFFFu) | (offs & 0xFF0000u) << 8;
        const int off3 = (int)(int8_t)(offs >> 24);
#pragma unroll
        for (int i = kPhase; i < 16; i += kStep) {
            const int ci = byte_of(c, i);
            const bool outside = (use_h && ((g.left && i < kStep) || (g.right && i >= 16 - kStep))) || (use_v && g.vert);
            const int r = outside ? ci : sao_apply_edge(ci, byte_of(a, i), byte_of(b, i), lo, off3);
            c[i >> 2] = (c[i >> 2] & ~(255u << (8 * (i & 3)))) | (uint32_t)r << (8 * (i & 3));
        }
    } else if (type == 1) {
#pragma unroll
        for (int i = kPhase; i < 16; i += kStep) {
            const int r = sao_apply_band(byte_of(c, i), (int)arg, offs);
            c[i >> 2] = (c[i >> 2] & ~(255u << (8 * (i & 3)))) | (uint32_t)r << (8 * (i & 3));
        }
    }
}

// ---- kernels: blockIdx.x walks the CTUs in raster order -------------------------------------------------------------------------
// statistics of a CTU into LDS bins; from there into d_stats (if given) and, kDecide, through the decision into d_param
template <bool kDecide>
__global__ __launch_bounds__(320) void sao_stats_kernel(const uint8_t *org, const uint8_t *dec, Frame f, int lambda_q4, int32_t *stats, x266_sao_t *param)
{
    __shared__ uint32_t luma[kLumaRows * kRowDwords];
    __shared__ uint32_t chroma[kChromaRows * kRowDwords];
    __shared__ int32_t bins[kCtuWords];
    const int t = (int)threadIdx.x, cy = (int)(blockIdx.x / (unsigned)f.ctus_x), cx = (int)(blockIdx.x - (unsigned)cy * (unsigned)f.ctus_x);
    const bool is_luma = t < 256;                                         // uniform per wave
    if (t < kCtuWords) bins[t] = 0;
    if (is_luma) load_halo<false>(f, dec, luma, cx, cy, t, 256);
    else         load_halo<true>(f, dec, chroma, cx, cy, t - 256, 64);
    __syncthreads();
    if (is_luma) {
        const int s = t >> 6, r = t & 63, x = 64 * cx + 16 * s, y = 64 * cy + r;
        const Segment g = make_segment(s, r, x, y, f.width, f.height, 16);
        uint32_t acc[1][16] = {};
        BandRun run[1] = {{-1, 0u}};
        v4i o = {0, 0, 0, 0};
        if (g.valid) o = load16<false>(org + luma_row_offset(f, x, y));
        stats_segment<1>(luma, g, o, acc, run, bins);
        stats_reduce<1>(acc, run, bins, t & 63);
    } else {
        uint32_t acc[2][16] = {};
        BandRun run[2] = {{-1, 0u}, {-1, 0u}};
#pragma unroll 1                                                          // rolled: unrolled, the kernel takes 187 VGPRs instead of 128
        for (int it = 0; it < 2; ++it) {
            const int q = t - 256 + 64 * it, s = q >> 5, r = q & 31, x = 32 * cx + 8 * s, y = 32 * cy + r;
            const Segment g = make_segment(s, r, x, y, f.width >> 1, f.height >> 1, 8);
            v4i o = {0, 0, 0, 0};
            if (g.valid) o = load16<false>(org + chroma_row_offset(f, x, y));
            stats_segment<2>(chroma, g, o, acc, run, bins + kSaoBins * 2);
        }
        stats_reduce<2>(acc, run, bins + kSaoBins * 2, t & 63);
    }
    __syncthreads();
    if (stats && t < kCtuWords) stats[(size_t)blockIdx.x * kCtuWords + (size_t)t] = bins[t];
    if (kDecide) {
        __shared__ DecideScratch scr;
        sao_decide(bins, scr, lambda_q4, param + (size_t)blockIdx.x * 3, t, t < 64);
    }
}

// four CTUs per workgroup, one per wave; a wave past the last CTU only keeps the barriers company
__global__ __launch_bounds__(256) void sao_decide_kernel(const int32_t *stats, unsigned n_ctu, int lambda_q4, x266_sao_t *param)
{
    __shared__ int32_t bins[4][kCtuWords];
    __shared__ DecideScratch scr[4];
    const int lane = (int)(threadIdx.x & 63);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ctu = blockIdx.x * 4 + wave;
    const bool active = ctu < n_ctu;
    if (active)
        for (int i = lane; i < kCtuWords; i += 64) bins[wave][i] = stats[(size_t)ctu * kCtuWords + (size_t)i];
    __syncthreads();
    sao_decide(bins[wave], scr[wave], lambda_q4, param + (size_t)ctu * 3, lane, active);
}

__global__ __launch_bounds__(320) void sao_apply_kernel(const uint8_t *in, uint8_t *out, Frame f, const x266_sao_t *param)
{
    __shared__ uint32_t luma[kLumaRows * kRowDwords];
    __shared__ uint32_t chroma[kChromaRows * kRowDwords];
    const int t = (int)threadIdx.x, cy = (int)(blockIdx.x / (unsigned)f.ctus_x), cx = (int)(blockIdx.x - (unsigned)cy * (unsigned)f.ctus_x);
    const bool is_luma = t < 256;                                         // uniform per wave
    const x266_sao_t *rec = param + (size_t)blockIdx.x * 3;
    if (is_luma) load_halo<false>(f, in, luma, cx, cy, t, 256);
    else         load_halo<true>(f, in, chroma, cx, cy, t - 256, 64);
    __syncthreads();
    if (is_luma) {
        const uint64_t rec_y = uniform_record(rec);
        const int s = t >> 6, r = t & 63, x = 64 * cx + 16 * s, y = 64 * cy + r;
        const Segment g = make_segment(s, r, x, y, f.width, f.height, 16);
        uint32_t c[4];
        seg16(luma, g.base, 0, c);
        apply_component<1, 0>(luma, g, rec_y, c);
        if (g.valid) store16<true>(out + luma_row_offset(f, x, y), v4i{(int)c[0], (int)c[1], (int)c[2], (int)c[3]});
    } else {
        const uint64_t rec_u = uniform_record(rec + 1), rec_v = uniform_record(rec + 2);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int q = t - 256 + 64 * it, s = q >> 5, r = q & 31, x = 32 * cx + 8 * s, y = 32 * cy + r;
            const Segment g = make_segment(s, r, x, y, f.width >> 1, f.height >> 1, 8);
            uint32_t c[4];
            seg16(chroma, g.base, 0, c);
            uint32_t v[4] = {c[0], c[1], c[2], c[3]};                     // V reads the unfiltered U bytes next to it, and the reverse
            apply_component<2, 0>(chroma, g, rec_u, c);
            apply_component<2, 1>(chroma, g, rec_v, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = (c[i] & 0x00FF00FFu) | (v[i] & 0xFF00FF00u);
            if (g.valid) store16<true>(out + chroma_row_offset(f, x, y), v4i{(int)c[0], (int)c[1], (int)c[2], (int)c[3]});
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

}  // namespace

// d_param NULL: statistics only; otherwise the decision runs in the same launch and d_stats may be NULL
hipError_t launch_sao_stats(const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, int lambda_q4, int32_t *d_stats,
                            x266_sao_t *d_param, hipStream_t stream)
{
    const Frame f = frame_of(width, height);
    const size_t n_ctu = (size_t)f.ctus_x * (size_t)((height + 63) / 64);
    if (n_ctu > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint8_t *org = reinterpret_cast<const uint8_t *>(d_org), *dec = reinterpret_cast<const uint8_t *>(d_dec);
    if (d_param) hipLaunchKernelGGL(sao_stats_kernel<true>, dim3((unsigned)n_ctu), dim3(320), 0, stream, org, dec, f, lambda_q4, d_stats, d_param);
    else         hipLaunchKernelGGL(sao_stats_kernel<false>, dim3((unsigned)n_ctu), dim3(320), 0, stream, org, dec, f, lambda_q4, d_stats, d_param);
    return hipGetLastError();
}

hipError_t launch_sao_decide(const int32_t *d_stats, size_t n_ctu, int lambda_q4, x266_sao_t *d_param, hipStream_t stream)
{
    if (n_ctu > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sao_decide_kernel, dim3((unsigned)((n_ctu + 3) / 4)), dim3(256), 0, stream, d_stats, (unsigned)n_ctu, lambda_q4, d_param);
    return hipGetLastError();
}

hipError_t launch_sao_apply(const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const x266_sao_t *d_param, hipStream_t stream)
{
    const Frame f = frame_of(width, height);
    const size_t n_ctu = (size_t)f.ctus_x * (size_t)((height + 63) / 64);
    if (n_ctu > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sao_apply_kernel, dim3((unsigned)n_ctu), dim3(320), 0, stream, reinterpret_cast<const uint8_t *>(d_in),
                       reinterpret_cast<uint8_t *>(d_out), f, d_param);
    return hipGetLastError();
}

}  // namespace x266
