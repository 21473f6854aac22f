// levels_kernels.hip -- the compact level stream (xLevelsPackGpu, xLevelsUnpackGpu): dense 1024-level regions <-> one record per region
// and a stream of significance maps and non-zero levels in coefficient-group scan order.  The contract is include/x266hip.h's, the
// tables and the CG arithmetic x266_levels.hpp's.
//
// One wave per region, lane g = CG bit g.  The region's 2 KiB cross an LDS slab of the wave's own: two 1 KiB-linear 16-byte accesses
// per lane on the global side (the quantiser's shape), four 8-byte LDS accesses per lane -- the four rows of its CG -- on the other.
// The lane's 16-bit map is formed in scan order, __ballot(map != 0) is cg_mask, a wave prefix sum of popcount(map) places the levels
// (wave_exclusive_sum, x266_lanes.hpp).
// Pack is three launches on one stream: count (records without offsets), scan (offsets and totals: ONE workgroup that walks the
// records kLevelsScanChunk at a time and carries a running total -- no workgroup ever waits for another, no position is handed out
// by an atomic, so the bytes depend on the data alone; the kernel is x266_levels.hpp's, shared with the motion stream), write (recomputes from the levels, builds the payload in LDS at the stream's
// own 16-byte phase and stores whole 16-byte chunks, single words only at the two ragged ends it shares with its neighbours).
// Unpack reads its maps straight from the stream, checks every extent against cap_words BEFORE any load, stages the levels through
// LDS the same way and writes the whole region, zeros included.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_levels.hpp"
#include "x266_quant.hpp"

namespace x266 {
namespace {

constexpr unsigned kLevelsWavesPerWg = 4;
constexpr unsigned kRegionBytes = kLevelsRegionWords * 2;
constexpr unsigned kPayloadSlabBytes = (kLevelsMaxWords + 8) * 2;          // up to 7 words of phase in front, whole 16-byte chunks
constexpr unsigned kLevelSlabBytes = (kLevelsRegionWords + 16) * 2;
static_assert(kPayloadSlabBytes % 16 == 0 && kLevelSlabBytes % 16 == 0, "slabs hold whole 16-byte chunks");
static_assert(sizeof(x266_level_region_t) == 32, "the record is 32 bytes");

__device__ __forceinline__ void region_to_lds(const int16_t *level, size_t r, unsigned lane, char *slab)
{
    const char *src = reinterpret_cast<const char *>(level) + r * kRegionBytes + lane * 16;
    const v4i a = load16<true>(src), b = load16<true>(src + 1024);
    *reinterpret_cast<v4i *>(slab + lane * 16) = a;
    *reinterpret_cast<v4i *>(slab + 1024 + lane * 16) = b;
}

// the 16 levels of the CG whose top-left level is `origin`, rows `n` levels apart: l[y * 4 + x]
__device__ __forceinline__ void cg_from_lds(const char *slab, unsigned origin, unsigned n, int (&l)[16])
{
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const uint2 w = *reinterpret_cast<const uint2 *>(slab + (origin + j * n) * 2);
        l[4 * j + 0] = (int)(int16_t)(w.x & 0xFFFFu);
        l[4 * j + 1] = (int)w.x >> 16;
        l[4 * j + 2] = (int)(int16_t)(w.y & 0xFFFFu);
        l[4 * j + 3] = (int)w.y >> 16;
    }
}

__device__ __forceinline__ void cg_to_lds(char *slab, unsigned origin, unsigned n, const int (&l)[16])
{
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        uint2 w;
        w.x = ((uint32_t)l[4 * j + 0] & 0xFFFFu) | ((uint32_t)l[4 * j + 1] << 16);
        w.y = ((uint32_t)l[4 * j + 2] & 0xFFFFu) | ((uint32_t)l[4 * j + 3] << 16);
        *reinterpret_cast<uint2 *>(slab + (origin + j * n) * 2) = w;
    }
}

// WRITE false: the count step, every field of the record but `offset`.  WRITE true: the write step, after the scan.
template <bool WRITE>
__global__ __launch_bounds__(64 * kLevelsWavesPerWg) void levels_pack_kernel(const int16_t *__restrict__ level, const uint8_t *__restrict__ cls,
                                                                            const uint32_t *__restrict__ nnz, x266_level_region_t *region,
                                                                            uint16_t *__restrict__ stream, size_t n_regions, uint64_t cap_words)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kLevelsWavesPerWg][kRegionBytes];
    __shared__ __attribute__((aligned(16))) char lds_payload[WRITE ? kLevelsWavesPerWg : 1][WRITE ? kPayloadSlabBytes : 16];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kLevelsWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;
    bool skip = !active;                                                   // wave-uniform: no level of the region is read
    uint64_t offset = 0;
    if (active && nnz && nnz[r] == 0) skip = true;
    if (WRITE && active) {
        const uint32_t n_words = region[r].n_words;
        offset = region[r].offset;
        if (n_words == 0 || offset > cap_words || n_words > cap_words - offset) skip = true;
    }
    char *slab = lds_region[wave_in_wg];
    if (!skip) region_to_lds(level, r, lane, slab);
    __syncthreads();
    int l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) l[i] = 0;
    if (!skip) {
        const unsigned k = cls ? (uniform_byte(cls, r) & 3u) : 3u;
        cg_from_lds(slab, level_cg_origin(k, lane), 4u << k, l);
    }
    uint32_t map = 0;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i) map |= (uint32_t)(l[level_scan4(i)] != 0) << i;
    const uint64_t cg_mask = __ballot(map != 0);
    const uint32_t count = (uint32_t)__popc(map), n_cg = (uint32_t)__popcll(cg_mask);
    const uint32_t n_nz = wave_sum(count);
    if (!WRITE) {
        uint32_t sum = 0, top = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t a = (uint32_t)(l[i] < 0 ? -l[i] : l[i]);
            sum += a;
            top = a > top ? a : top;
        }
        sum = wave_sum(sum);
        top = wave_max(top);
        if (active && lane == 0) {
            x266_level_region_t *rec = region + r;
            rec->cg_mask = cg_mask;
            rec->n_words = n_cg + n_nz;
            rec->n_nz = n_nz;
            rec->sum_abs = sum;
            rec->max_abs = top;
        }
        return;
    }
    // the payload in LDS, word `phase` of the slab = word `offset` of the stream: slab chunk c is the stream's 16-byte chunk
    uint16_t *pay = reinterpret_cast<uint16_t *>(lds_payload[WRITE ? wave_in_wg : 0]);
    const unsigned phase = (unsigned)(offset & 7u);
    const uint32_t below = wave_exclusive_sum(count, lane);                 // every lane takes part in the shuffles
    if (map) {
        pay[phase + (unsigned)__popcll(cg_mask & ((1ull << lane) - 1ull))] = (uint16_t)map;
        unsigned at = phase + n_cg + below;
#pragma unroll
        for (unsigned i = 0; i < 16; ++i)
            if ((map >> i) & 1u) pay[at++] = (uint16_t)l[level_scan4(i)];
    }
    __syncthreads();
    const unsigned n_words = n_cg + n_nz;
    if (skip || n_words == 0 || n_words > cap_words - offset) return;       // as counted; held against the capacity again all the same
    uint16_t *dst = stream + (offset - phase);                              // 16-byte aligned: d_stream is, and offset - phase is a multiple of 8
    const unsigned n_chunks = (phase + n_words + 7u) >> 3;
    for (unsigned c = lane; c < n_chunks; c += 64) {
        const unsigned lo = c * 8;
        if (lo >= phase && lo + 8 <= phase + n_words) {
            *reinterpret_cast<v4i *>(dst + lo) = *reinterpret_cast<const v4i *>(pay + lo);
        } else {
            for (unsigned w = lo; w < lo + 8; ++w)
                if (w >= phase && w < phase + n_words) dst[w] = pay[w];
        }
    }
}

__global__ __launch_bounds__(64 * kLevelsWavesPerWg) void levels_unpack_kernel(int16_t *__restrict__ level, const uint8_t *__restrict__ cls,
                                                                              uint32_t *__restrict__ nnz, const x266_level_region_t *__restrict__ region,
                                                                              const uint16_t *__restrict__ stream, size_t n_regions, uint64_t cap_words)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kLevelsWavesPerWg][kRegionBytes];
    __shared__ __attribute__((aligned(16))) char lds_levels[kLevelsWavesPerWg][kLevelSlabBytes];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kLevelsWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;
    uint64_t cg_mask = 0, offset = 0;
    if (active) {
        cg_mask = region[r].cg_mask;
        offset = region[r].offset;
    }
    const uint32_t n_cg = (uint32_t)__popcll(cg_mask);
    bool ok = active && offset <= cap_words && n_cg <= cap_words - offset;   // the maps lie inside the stream
    uint32_t map = 0;
    if (ok && ((cg_mask >> lane) & 1ull)) map = stream[offset + (unsigned)__popcll(cg_mask & ((1ull << lane) - 1ull))];
    uint32_t count = (uint32_t)__popc(map);
    uint32_t n_nz = wave_sum(count);
    ok = ok && n_nz <= cap_words - offset - n_cg;                            // ... and so do the levels they announce
    if (!ok) {
        map = 0;
        count = 0;
        n_nz = 0;
    }
    const uint32_t below = wave_exclusive_sum(count, lane);
    // the levels into LDS, word `phase` of the slab = the first level's word of the stream; only words of this payload are read
    const uint64_t first = offset + n_cg;
    const unsigned phase = (unsigned)(first & 7u);
    uint16_t *lv = reinterpret_cast<uint16_t *>(lds_levels[wave_in_wg]);
    if (n_nz) {
        const uint16_t *src = stream + (first - phase);
        const unsigned n_chunks = (phase + n_nz + 7u) >> 3;
        for (unsigned c = lane; c < n_chunks; c += 64) {
            const unsigned lo = c * 8;
            if (lo >= phase && lo + 8 <= phase + n_nz) {
                *reinterpret_cast<v4i *>(lv + lo) = *reinterpret_cast<const v4i *>(src + lo);
            } else {
                for (unsigned w = lo; w < lo + 8; ++w)
                    if (w >= phase && w < phase + n_nz) lv[w] = src[w];
            }
        }
    }
    __syncthreads();
    int l[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) l[i] = 0;
    unsigned at = phase + below;
#pragma unroll
    for (unsigned i = 0; i < 16; ++i)
        if ((map >> i) & 1u) l[level_scan4(i)] = (int)(int16_t)lv[at++];
    char *slab = lds_region[wave_in_wg];
    const unsigned k = (active && cls) ? (uniform_byte(cls, r) & 3u) : 3u;
    cg_to_lds(slab, level_cg_origin(k, lane), 4u << k, l);
    __syncthreads();
    if (!active) return;
    char *dst = reinterpret_cast<char *>(level) + r * kRegionBytes + lane * 16;
    store16<true>(dst, *reinterpret_cast<const v4i *>(slab + lane * 16));
    store16<true>(dst + 1024, *reinterpret_cast<const v4i *>(slab + 1024 + lane * 16));
    if (nnz && lane == 0) nnz[r] = n_nz;
}

}  // namespace

unsigned levels_scan_chunk() { return kLevelsScanChunk; }

hipError_t launch_levels_pack(const x266_levels_t &p, hipStream_t stream)
{
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kLevelsWavesPerWg, &wgs)) return e;
    const dim3 block(64 * kLevelsWavesPerWg);
    if (p.n_regions) {
        hipLaunchKernelGGL(levels_pack_kernel<false>, dim3(wgs), block, 0, stream, p.d_level, p.d_class, p.d_nnz, p.d_region, (uint16_t *)nullptr, p.n_regions,
                           (uint64_t)0);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(levels_scan_kernel<x266_level_region_t>, dim3(1), dim3(kLevelsScanChunk), 0, stream, p.d_region, p.n_regions, p.cap_words, p.d_total);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.n_regions && p.cap_words && p.d_stream)
        hipLaunchKernelGGL(levels_pack_kernel<true>, dim3(wgs), block, 0, stream, p.d_level, p.d_class, p.d_nnz, p.d_region, p.d_stream, p.n_regions, p.cap_words);
    return hipGetLastError();
}

hipError_t launch_levels_unpack(const x266_levels_t &p, hipStream_t stream)
{
    if (p.n_regions == 0) return hipSuccess;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kLevelsWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(levels_unpack_kernel, dim3(wgs), dim3(64 * kLevelsWavesPerWg), 0, stream, p.d_level, p.d_class, p.d_nnz, p.d_region, p.d_stream,
                       p.n_regions, p.cap_words);
    return hipGetLastError();
}

}  // namespace x266
