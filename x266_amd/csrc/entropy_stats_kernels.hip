// entropy_stats_kernels.hip -- the per-context bin statistics (xEntropyStatsLevelsGpu, xEntropyStatsSideGpu).  The contract is
// include/x266hip.h's ("per-context bin statistics on the device"); the definition both are held against is the coders' own syntax walks
// run with the counting sink of x266_entropy.hpp (xEntropyCountRegion, xEntropyCountSideCtu).
//
// Levels.  Which context a bin goes to and whether it is 0 or 1 depends on the levels alone, so nothing here is a coder and nothing is
// serial.  One wave takes a region at a time, lane g = CG bit g (level_cg_origin, as the encoder's cg_mask).  A lane loads the four
// 8-byte rows of its CG straight from the region (each byte of the region is read once, by one lane) and forms three 16-bit maps in SCAN
// order: sig (l != 0), |l| > 1, |l| > 2.  __ballot(sig != 0) is the region's coded-CG mask; a lane cuts its own block's bits out of it:
//     cbf    the lane of CG 0 of a block: one bin, the block's bits are not all zero
//     last   the lane of the block's highest coded CG s_p: i_p = the top bit of sig, (u, v) from the CG's origin and scan4(i_p), the
//            groups g(u), g(v); context i of a coordinate gets a one for i < g and a zero for i == g < 2n - 1
//     cgf    the lanes with 0 < s < s_p: one bin, sig != 0
//     sig    the lanes of CG 0 and of coded CGs: 16 bins, in CG s_p the i_p below the last position; ones popcount(sig & bins), zeros
//            popcount(~sig & bins); position class 0 is bit 0 of CG 0, class 1 the other bits of CG 0, class 2 every other CG
//     gt1    popcount(sig) bins, popcount(|l| > 1) ones;   gt2   popcount(|l| > 1) bins, popcount(|l| > 2) ones
// Every non-zero level of a block is walked by the coder (it lies in a coded CG at or below s_p, in CG s_p at or below i_p), so gt1 and
// gt2 need no condition.  The lanes keep their counts in registers over the 8 regions a wave takes and reduce ONCE, at the end; a row of
// X266_ENTROPY_STATS_REGIONS = 32 regions is a workgroup of 4 waves, whose sums meet in LDS and are added in the order 0 .. 3.
// The two traps of that shape:
//   * the size k changes from region to region, so "the 25 accumulators of size k" is a run-time row, and an indexed register array lives in
//     scratch.  k is wave-uniform: the region's bins are formed size-blind into one RegionBins, and a uniform switch adds them to one of
//     four NAMED accumulator sets.  Zeros and ones of a context share a register, 16 bits each (a lane adds at most 16 per region and
//     context, 128 per row; a wave's sum stays below 2^13).
//   * the last position's context is a run-time index too.  A lane does not index: it adds 1 to field g of a histogram of g, ten 10-bit
//     fields in four registers per coordinate (a shift by a run-time amount, the register chosen by four compares); the one and zero bins
//     of contexts 0 .. 8 follow from the histogram at the end of the row: ones(i) = sum of hist(g) over g > i, zeros(i) = hist(i) for
//     i < 2n - 1.  A lane is the last CG of at most one block per region: a field holds at most 8, a wave's sum at most 512.
// Side information.  One lane per CTU as the side coder: entropy_side_canon, then the syntax's own walk (entropy_side_encode_ctu) with
// EntropyCounter as its sink; the 32 counters of a lane are run-time indexed and so sit in LDS, counter-major with the lane the fast index
// (32 lanes, 32 banks).  A row is the 64 CTUs of a one-wave workgroup.
// Totals: one workgroup adds the rows in ascending order into 64-bit counters (as quality_totals_kernel does); no atomics anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_entropy.hpp"
#include "x266_entropy_side.hpp"
#include "x266_lanes.hpp"
#include "x266_levels.hpp"

namespace x266 {
namespace {

constexpr unsigned kStatsWaves = 4;                                          // waves of a row's workgroup
constexpr unsigned kStatsRegionsPerWave = X266_ENTROPY_STATS_REGIONS / kStatsWaves;
constexpr unsigned kStatsCounters = 2 * kEntropyContexts, kStatsSizeCounters = 2 * kEntropyCtxPerSize;
constexpr unsigned kSideStatsCounters = 2 * kEntropySideContexts;
constexpr unsigned kStatsTotalsThreads = 1024;
static_assert(X266_ENTROPY_STATS_REGIONS % kStatsWaves == 0 && kStatsRegionsPerWave * 16 * 64 < 65536, "16-bit halves hold a wave's sum");
static_assert(kStatsRegionsPerWave * 64 < 1024, "10-bit histogram fields hold a wave's sum");
static_assert(X266_ENTROPY_SIDE_STATS_CTUS == 64, "a row of the side call is one wave, one lane per CTU");

// scan position of raster position yx of a 4x4 CG, and the raster positions of the 16 scan positions in one word, 4 bits each
constexpr unsigned stats_pos4(unsigned yx)
{
    unsigned at = 0;
    for (unsigned i = 0; i < 16; ++i)
        if (level_scan4(i) == yx) at = i;
    return at;
}
constexpr uint64_t stats_scan4_word()
{
    uint64_t w = 0;
    for (unsigned i = 0; i < 16; ++i) w |= (uint64_t)level_scan4(i) << (4 * i);
    return w;
}

struct CgRows {
    uint2 row[4];
};
// the 16 levels of the CG at `origin` of region r, rows `size` levels apart: 8-byte aligned, because origins and sizes are multiples of 4
__device__ __forceinline__ CgRows stats_load_cg(const int16_t *level, size_t r, unsigned origin, unsigned size, bool read)
{
    CgRows c;
    const char *p = reinterpret_cast<const char *>(level) + r * (kLevelsRegionWords * 2) + origin * 2u;
#pragma unroll
    for (unsigned y = 0; y < 4; ++y) c.row[y] = read ? *reinterpret_cast<const uint2 *>(p + y * size * 2u) : make_uint2(0u, 0u);
    return c;
}

// what one region adds for this lane; zeros in the low half, ones in the high half
struct RegionBins {
    uint32_t cbf, cgf, sig0, sig1, sig2, gt1, gt2;
    unsigned gx, gy;
    bool last;
};
__device__ __forceinline__ uint32_t stats_pair(unsigned zeros, unsigned ones) { return zeros | ones << 16; }

__device__ __forceinline__ RegionBins stats_region_bins(const CgRows &c, unsigned k, unsigned lane, unsigned origin)
{
    unsigned sig = 0, m1 = 0, m2 = 0;
#pragma unroll
    for (unsigned yx = 0; yx < 16; ++yx) {
        const uint32_t w = (yx & 2u) ? c.row[yx >> 2].y : c.row[yx >> 2].x;
        const int l = (int16_t)((yx & 1u) ? w >> 16 : w & 0xFFFFu);
        const unsigned a = (unsigned)(l < 0 ? -l : l), i = stats_pos4(yx);
        sig |= (unsigned)(a != 0u) << i;
        m1 |= (unsigned)(a > 1u) << i;
        m2 |= (unsigned)(a > 2u) << i;
    }
    const uint64_t cg_mask = __ballot(sig != 0u);
    const unsigned per_log = 2u * k, blk = lane >> per_log, s = lane & ((1u << per_log) - 1u);
    const uint64_t cgs = (cg_mask >> (blk << per_log)) & (per_log == 6u ? ~0ull : (1ull << (1u << per_log)) - 1ull);
    const bool any = cgs != 0;
    const unsigned sp = any ? 63u - (unsigned)__builtin_clzll(cgs) : 0u;
    RegionBins b;
    b.last = any && s == sp;                                                // then sig != 0: CG s_p is a coded one
    const unsigned ip = b.last ? 31u - (unsigned)__builtin_clz(sig | 1u) : 0u;
    b.cbf = s == 0u ? stats_pair(!any, any) : 0u;
    b.cgf = any && s > 0u && s < sp ? stats_pair(sig == 0u, sig != 0u) : 0u;
    const bool walked = any && (s == 0u || sig != 0u);                      // CG 0 is implied coded; a coded CG is at or below s_p
    const unsigned bins = !walked ? 0u : b.last ? (1u << ip) - 1u : 0xFFFFu, ones = sig & bins, zeros = ~sig & bins;
    b.sig0 = s == 0u ? stats_pair(zeros & 1u, ones & 1u) : 0u;
    b.sig1 = s == 0u ? stats_pair((unsigned)__popc(zeros & 0xFFFEu), (unsigned)__popc(ones & 0xFFFEu)) : 0u;
    b.sig2 = s != 0u ? stats_pair((unsigned)__popc(zeros), (unsigned)__popc(ones)) : 0u;
    const unsigned n_sig = (unsigned)__popc(sig), n_1 = (unsigned)__popc(m1), n_2 = (unsigned)__popc(m2);
    b.gt1 = stats_pair(n_sig - n_1, n_1);
    b.gt2 = stats_pair(n_1 - n_2, n_2);
    const unsigned yx = (unsigned)(stats_scan4_word() >> (4u * ip)) & 15u, n = k + 2u;
    const unsigned org = origin - (blk << (2u * n));                        // inside the block: blocks are N * N levels apart
    b.gx = entropy_last_group((org & ((1u << n) - 1u)) + (yx & 3u));
    b.gy = entropy_last_group((org >> n) + (yx >> 2));
    return b;
}

// the accumulators of one block size
struct SizeBins {
    uint32_t cbf, cgf, sig0, sig1, sig2, gt1, gt2;
    uint32_t hx[4], hy[4];                                                  // field g % 3 of register g / 3: the lanes that had g(u), g(v) = g
};
__device__ __forceinline__ void stats_hist_add(uint32_t (&h)[4], bool on, unsigned g)
{
    const uint32_t inc = on ? 1u << (10u * (g % 3u)) : 0u;
    const unsigned reg = g / 3u;
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) h[j] += reg == j ? inc : 0u;
}
__device__ __forceinline__ void stats_add(SizeBins &a, const RegionBins &b)
{
    a.cbf += b.cbf;
    a.cgf += b.cgf;
    a.sig0 += b.sig0;
    a.sig1 += b.sig1;
    a.sig2 += b.sig2;
    a.gt1 += b.gt1;
    a.gt2 += b.gt2;
    stats_hist_add(a.hx, b.last, b.gx);
    stats_hist_add(a.hy, b.last, b.gy);
}

// the wave's 50 counters of size k into out[0 .. 50): every lane calls it, lane 0 writes
__device__ __forceinline__ void stats_emit_pair(uint32_t *out, unsigned ctx, uint32_t packed, unsigned lane)
{
    const uint32_t v = wave_sum(packed);
    if (lane == 0) {
        out[2u * ctx] = v & 0xFFFFu;
        out[2u * ctx + 1u] = v >> 16;
    }
}
__device__ __forceinline__ void stats_emit_last(uint32_t *out, unsigned first_ctx, const uint32_t (&h)[4], unsigned k, unsigned lane)
{
    uint32_t f[12];
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const uint32_t v = wave_sum(h[j]);
#pragma unroll
        for (unsigned t = 0; t < 3; ++t) f[3 * j + t] = (v >> (10u * t)) & 1023u;
    }
    const unsigned top = 2u * k + 3u;                                       // 2n - 1
    uint32_t above = 0;                                                     // lanes with g > i
#pragma unroll
    for (unsigned i = 9; i-- > 0;) {
        above += f[i + 1];
        if (lane == 0) {
            out[2u * (first_ctx + i)] = i < top ? f[i] : 0u;
            out[2u * (first_ctx + i) + 1u] = above;
        }
    }
}
__device__ __forceinline__ void stats_emit(uint32_t *out, const SizeBins &a, unsigned k, unsigned lane)
{
    stats_emit_pair(out, kCtxCbf, a.cbf, lane);
    stats_emit_last(out, kCtxLastX, a.hx, k, lane);
    stats_emit_last(out, kCtxLastY, a.hy, k, lane);
    stats_emit_pair(out, kCtxCgf, a.cgf, lane);
    stats_emit_pair(out, kCtxSig, a.sig0, lane);
    stats_emit_pair(out, kCtxSig + 1, a.sig1, lane);
    stats_emit_pair(out, kCtxSig + 2, a.sig2, lane);
    stats_emit_pair(out, kCtxGt1, a.gt1, lane);
    stats_emit_pair(out, kCtxGt2, a.gt2, lane);
}

__global__ __launch_bounds__(64 * kStatsWaves) void entropy_stats_levels_kernel(const int16_t *__restrict__ level, const uint8_t *__restrict__ cls,
                                                                              const uint32_t *__restrict__ nnz, uint32_t *__restrict__ part, size_t n_regions)
{
    __shared__ uint32_t lds_part[kStatsWaves][kStatsCounters];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const size_t first = (size_t)blockIdx.x * X266_ENTROPY_STATS_REGIONS + wave * kStatsRegionsPerWave;
    // lane i < 8 fetches what the wave needs to know of its region i: bit 0 it exists, bit 1 its levels count, bits 2..3 its size
    unsigned about = 0;
    if (lane < kStatsRegionsPerWave && first + lane < n_regions) {
        const size_t r = first + lane;
        about = 1u | ((!nnz || nnz[r] != 0u) ? 2u : 0u) | (cls ? (cls[r] & 3u) : 3u) << 2;
    }
    const unsigned origin[4] = {level_cg_origin(0, lane), level_cg_origin(1, lane), level_cg_origin(2, lane), level_cg_origin(3, lane)};
    SizeBins a0 = {}, a1 = {}, a2 = {}, a3 = {};
    unsigned k_next = ((unsigned)__builtin_amdgcn_readlane((int)about, 0) >> 2) & 3u;
    unsigned org_next = k_next == 0u ? origin[0] : k_next == 1u ? origin[1] : k_next == 2u ? origin[2] : origin[3];
    CgRows next = stats_load_cg(level, first, org_next, 4u << k_next, ((unsigned)__builtin_amdgcn_readlane((int)about, 0) & 3u) == 3u);
#pragma unroll
    for (unsigned i = 0; i < kStatsRegionsPerWave; ++i) {
        const unsigned here = (unsigned)__builtin_amdgcn_readlane((int)about, i), k = k_next, org = org_next;
        const CgRows cur = next;
        if (i + 1 < kStatsRegionsPerWave) {                                 // the next region's rows fly over this region's arithmetic
            const unsigned then = (unsigned)__builtin_amdgcn_readlane((int)about, i + 1 < kStatsRegionsPerWave ? i + 1 : i);
            k_next = (then >> 2) & 3u;
            org_next = k_next == 0u ? origin[0] : k_next == 1u ? origin[1] : k_next == 2u ? origin[2] : origin[3];
            next = stats_load_cg(level, first + i + 1, org_next, 4u << k_next, (then & 3u) == 3u);
        }
        if (!(here & 1u)) continue;                                         // wave-uniform: past the last region
        const RegionBins b = stats_region_bins(cur, k, lane, org);
        switch (k) {                                                        // wave-uniform
        case 0: stats_add(a0, b); break;
        case 1: stats_add(a1, b); break;
        case 2: stats_add(a2, b); break;
        default: stats_add(a3, b); break;
        }
    }
    uint32_t *mine = lds_part[wave];
    stats_emit(mine, a0, 0, lane);
    stats_emit(mine + kStatsSizeCounters, a1, 1, lane);
    stats_emit(mine + 2 * kStatsSizeCounters, a2, 2, lane);
    stats_emit(mine + 3 * kStatsSizeCounters, a3, 3, lane);
    __syncthreads();
    if (tid < kStatsCounters) {
        uint32_t all = 0;
#pragma unroll
        for (unsigned w = 0; w < kStatsWaves; ++w) all += lds_part[w][tid];
        part[(size_t)blockIdx.x * kStatsCounters + tid] = all;
    }
}

struct SideStatsArrays {
    const uint8_t *kind, *mode, *cls, *qp;
    const uint32_t *nnz;
};

__global__ __launch_bounds__(X266_ENTROPY_SIDE_STATS_CTUS) void entropy_stats_side_kernel(const SideStatsArrays in, uint32_t *__restrict__ part, size_t n_ctu, int qp,
                                                                                            int chroma_qp_offset)
{
    __shared__ uint32_t lds_count[kSideStatsCounters * 64];
    const unsigned lane = threadIdx.x;
    const size_t c = (size_t)blockIdx.x * 64 + lane;
#pragma unroll
    for (unsigned i = 0; i < kSideStatsCounters; ++i) lds_count[i * 64 + lane] = 0;
    if (c < n_ctu) {
        const size_t r = 6 * c;
        const EntropySideCtu s = entropy_side_canon(in.kind ? in.kind + r : nullptr, in.mode ? in.mode + r : nullptr, in.cls ? in.cls + r : nullptr,
                                                    in.qp ? in.qp + r : nullptr, in.nnz ? in.nnz + r : nullptr, qp, chroma_qp_offset);
        uint16_t *ctx = reinterpret_cast<uint16_t *>(lds_count);            // the walk's addresses: the sink reads and writes no context
        EntropyCounter<uint32_t, 64> e = {lds_count + lane, ctx};
        entropy_side_encode_ctu(e, s, ctx, 1u, qp, chroma_qp_offset);
    }
    uint32_t mine = 0;                                                      // lane i ends up with counter i of the row
#pragma unroll
    for (unsigned i = 0; i < kSideStatsCounters; ++i) {
        const uint32_t v = wave_sum(lds_count[i * 64 + lane]);
        mine = lane == i ? v : mine;
    }
    if (lane < kSideStatsCounters) part[(size_t)blockIdx.x * kSideStatsCounters + lane] = mine;
}

// counts[c] = the sum of part[j][c] over the rows: thread group g takes the rows g, g + kGroups, ...; the groups' sums meet in LDS and are
// added in the order 0 .. kGroups - 1.  rows == 0 writes zeros and reads nothing.
template <unsigned N>
__global__ __launch_bounds__(kStatsTotalsThreads) void entropy_stats_totals_kernel(const uint32_t *__restrict__ part, size_t rows, uint64_t *__restrict__ counts)
{
    constexpr unsigned kGroups = kStatsTotalsThreads / N;
    __shared__ uint64_t lds_sum[kGroups][N];
    const unsigned tid = threadIdx.x, group = tid / N, c = tid % N;
    if (group < kGroups) {
        uint64_t sum = 0;
        for (size_t j = group; j < rows; j += kGroups) sum += part[j * N + c];
        lds_sum[group][c] = sum;
    }
    __syncthreads();
    if (tid < N) {
        uint64_t all = 0;
#pragma unroll
        for (unsigned g = 0; g < kGroups; ++g) all += lds_sum[g][tid];
        counts[tid] = all;
    }
}

size_t stats_rows(size_t n, size_t per_row) { return n / per_row + (n % per_row != 0); }

}  // namespace

hipError_t launch_entropy_stats_levels(const x266_entropy_stats_t &p, hipStream_t stream)
{
    const size_t rows = stats_rows(p.n_regions, X266_ENTROPY_STATS_REGIONS);
    if (rows > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (rows) {
        hipLaunchKernelGGL(entropy_stats_levels_kernel, dim3((unsigned)rows), dim3(64 * kStatsWaves), 0, stream, p.d_level, p.d_class, p.d_nnz, p.d_part, p.n_regions);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(entropy_stats_totals_kernel<kStatsCounters>, dim3(1), dim3(kStatsTotalsThreads), 0, stream, (const uint32_t *)p.d_part, rows, p.d_counts);
    return hipGetLastError();
}

hipError_t launch_entropy_stats_side(const x266_entropy_side_stats_t &p, hipStream_t stream)
{
    const size_t rows = stats_rows(p.n_ctu, X266_ENTROPY_SIDE_STATS_CTUS);
    if (rows > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (rows) {
        hipLaunchKernelGGL(entropy_stats_side_kernel, dim3((unsigned)rows), dim3(X266_ENTROPY_SIDE_STATS_CTUS), 0, stream,
                           SideStatsArrays{p.d_kind, p.d_mode, p.d_class, p.d_qp, p.d_nnz}, p.d_part, p.n_ctu, p.qp, p.chroma_qp_offset);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(entropy_stats_totals_kernel<kSideStatsCounters>, dim3(1), dim3(kStatsTotalsThreads), 0, stream, (const uint32_t *)p.d_part, rows, p.d_counts);
    return hipGetLastError();
}

}  // namespace x266
