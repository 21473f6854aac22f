// entropy_kernels.hip -- the entropy coder of the level stream (xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu): dense 1024-level regions
// <-> one record per region and one range-coded substream per region.  The contract is include/x266hip.h's, the coder, the syntax and the
// tables x266_entropy.hpp's -- the very functions the host helpers run.
//
// One wave per region.  The region's 2 KiB cross an LDS slab of the wave's own with two 16-byte accesses per lane, as in
// levels_kernels.hip; lane g forms the map of CG g, __ballot(map != 0) is the coded-CG mask that tells the coder which CGs to read at all.
// The coder itself is one lane wide -- an arithmetic coder's state is a chain from the first bin to the last -- and runs on lane 0 over the
// slab, with its 25 contexts in LDS (an indexed array in registers would live in scratch).  The chip is filled by waves, not by lanes:
// 12 240 regions at 3840 x 2176.
// Encode is three launches on one stream: count (records without offsets; the sink stores nothing, so no payload slab exists), scan (the
// level stream's offset scan, x266_levels.hpp), write (codes again, the bytes into an LDS slab at the stream's own 16-byte phase, then whole
// 16-byte chunks, single words only at the two ragged ends a substream shares with its neighbours).
// Decode checks offset and n_bytes against cap_words BEFORE any load, stages the substream through LDS the same way, decodes on lane 0
// into a zeroed region slab and writes the whole region, zeros included; a malformed region is cleared again.
// The slab copy (substream_copy) is x266_entropy.hpp's: entropy_motion_kernels.hip, the motion stream's coder of the same shape, shares it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_entropy.hpp"
#include "x266_lanes.hpp"
#include "x266_levels.hpp"

namespace x266 {
namespace {

constexpr unsigned kEntropyWavesPerWg = 4;
constexpr unsigned kRegionBytes = kLevelsRegionWords * 2;
constexpr unsigned kStreamSlabBytes = kEntropyMaxBytes + 16;               // up to 7 words of phase in front, a pad byte, whole 16-byte chunks
constexpr unsigned kCtxSlab = 32;                                           // 25 contexts
constexpr uint32_t kMalformed = 0xFFFFFFFFu;
static_assert(kStreamSlabBytes % 16 == 0, "slabs hold whole 16-byte chunks");
static_assert(sizeof(x266_entropy_region_t) == 32 && offsetof(x266_entropy_region_t, offset) == offsetof(x266_level_region_t, offset) &&
                  offsetof(x266_entropy_region_t, n_words) == offsetof(x266_level_region_t, n_words),
              "the offset scan reads n_words and writes offset where the level record has them");

__device__ __forceinline__ void region_to_lds(const int16_t *level, size_t r, unsigned lane, char *slab)
{
    const char *src = reinterpret_cast<const char *>(level) + r * kRegionBytes + lane * 16;
    const v4i a = load16<true>(src), b = load16<true>(src + 1024);
    *reinterpret_cast<v4i *>(slab + lane * 16) = a;
    *reinterpret_cast<v4i *>(slab + 1024 + lane * 16) = b;
}

// is any of the 16 levels of the CG whose top-left level is `origin`, rows `n` levels apart, non-zero
__device__ __forceinline__ unsigned cg_count_from_lds(const char *slab, unsigned origin, unsigned n)
{
    unsigned count = 0;
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const uint2 w = *reinterpret_cast<const uint2 *>(slab + (origin + j * n) * 2);
        count += ((w.x & 0xFFFFu) != 0) + ((w.x >> 16) != 0) + ((w.y & 0xFFFFu) != 0) + ((w.y >> 16) != 0);
    }
    return count;
}

// WRITE false: the count step, every field of the record but `offset`.  WRITE true: the write step, after the scan.
template <bool WRITE>
__global__ __launch_bounds__(64 * kEntropyWavesPerWg) void entropy_encode_kernel(const int16_t *__restrict__ level, const uint8_t *__restrict__ cls,
                                                                                const uint32_t *__restrict__ nnz, x266_entropy_region_t *region,
                                                                                uint16_t *__restrict__ stream, size_t n_regions, uint64_t cap_words,
                                                                                const EntropyInit init)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kEntropyWavesPerWg][kRegionBytes];
    __shared__ __attribute__((aligned(16))) char lds_stream[WRITE ? kEntropyWavesPerWg : 1][WRITE ? kStreamSlabBytes : 16];
    __shared__ uint16_t lds_ctx[kEntropyWavesPerWg][kCtxSlab];
    __shared__ uint32_t lds_bytes[kEntropyWavesPerWg];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kEntropyWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;
    bool skip = !active;                                                   // wave-uniform: no level of the region is read
    uint64_t offset = 0;
    uint32_t n_words = 0;
    if (active && nnz && nnz[r] == 0) skip = true;
    if (WRITE && active) {
        n_words = region[r].n_words;
        offset = region[r].offset;
        if (n_words == 0 || offset > cap_words || n_words > cap_words - offset) skip = true;
    }
    char *slab = lds_region[wave_in_wg];
    uint16_t *ctx = lds_ctx[wave_in_wg];
    if (!skip) region_to_lds(level, r, lane, slab);
    const unsigned k = (active && cls) ? (uniform_byte(cls, r) & 3u) : 3u;
    if (lane < kEntropyCtxPerSize) ctx[lane] = init.p[k * kEntropyCtxPerSize + lane];
    __syncthreads();
    const unsigned count = skip ? 0u : cg_count_from_lds(slab, level_cg_origin(k, lane), 4u << k);
    const uint64_t cg_mask = __ballot(count != 0);
    const uint32_t n_nz = wave_sum(count);
    const unsigned phase = (unsigned)(offset & 7u);
    uint8_t *pay = reinterpret_cast<uint8_t *>(lds_stream[WRITE ? wave_in_wg : 0]) + phase * 2;
    if (lane == 0 && active && (!WRITE || !skip)) {                         // the serial section: the coder's state is one chain
        EntropyEnc e;
        entropy_enc_start(e, WRITE ? pay : nullptr, WRITE ? kEntropyMaxBytes : 0u);
        entropy_encode_region(e, reinterpret_cast<const int16_t *>(slab), k, cg_mask, ctx);
        const uint32_t n_bytes = entropy_enc_finish(e);
        if (WRITE) {
            if (n_bytes <= kEntropyMaxBytes && (n_bytes & 1u)) pay[n_bytes] = 0;   // the pad byte; the slab has room for it behind the last byte
            lds_bytes[wave_in_wg] = n_bytes;
        } else {
            x266_entropy_region_t *rec = region + r;
            rec->ctx_bins = e.ctx_bins;
            rec->bypass_bins = e.bypass_bins;
            rec->n_words = (n_bytes + 1u) >> 1;
            rec->n_bytes = n_bytes;
            rec->n_nz = n_nz;
            rec->reserved = 0;
        }
    }
    if (!WRITE) return;
    __syncthreads();
    if (skip) return;
    const uint32_t n_bytes = lds_bytes[wave_in_wg];
    if (n_bytes > kEntropyMaxBytes || ((n_bytes + 1u) >> 1) != n_words) return;   // as counted; held against the record all the same
    const uint16_t *src = reinterpret_cast<const uint16_t *>(lds_stream[wave_in_wg]);
    uint16_t *dst = stream + (offset - phase);                              // 16-byte aligned: d_stream is, and offset - phase is a multiple of 8
    substream_copy(dst, src, phase, n_words, lane);
}

__global__ __launch_bounds__(64 * kEntropyWavesPerWg) void entropy_decode_kernel(int16_t *__restrict__ level, const uint8_t *__restrict__ cls,
                                                                                uint32_t *__restrict__ nnz, const x266_entropy_region_t *__restrict__ region,
                                                                                const uint16_t *__restrict__ stream, size_t n_regions, uint64_t cap_words,
                                                                                const EntropyInit init)
{
    __shared__ __attribute__((aligned(16))) char lds_region[kEntropyWavesPerWg][kRegionBytes];
    __shared__ __attribute__((aligned(16))) char lds_stream[kEntropyWavesPerWg][kStreamSlabBytes];
    __shared__ uint16_t lds_ctx[kEntropyWavesPerWg][kCtxSlab];
    __shared__ uint32_t lds_count[kEntropyWavesPerWg];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = (size_t)blockIdx.x * kEntropyWavesPerWg + wave_in_wg;
    const bool active = r < n_regions;
    uint64_t offset = 0;
    uint32_t n_bytes = 0;
    if (active) {
        offset = region[r].offset;
        n_bytes = region[r].n_bytes;
    }
    uint32_t n_words = (n_bytes >> 1) + (n_bytes & 1u);                      // no wrap at 2^32 - 1
    const bool ok = active && n_bytes <= kEntropyMaxBytes && offset <= cap_words && n_words <= cap_words - offset;
    if (!ok) {
        offset = 0;
        n_bytes = n_words = 0;
    }
    // the substream into LDS, word `phase` of the slab = word `offset` of the stream; only words of this substream are read
    const unsigned phase = (unsigned)(offset & 7u);
    uint16_t *pay = reinterpret_cast<uint16_t *>(lds_stream[wave_in_wg]);
    if (n_words) {
        const uint16_t *src = stream + (offset - phase);
        substream_copy(pay, src, phase, n_words, lane);
    }
    char *slab = lds_region[wave_in_wg];
    uint16_t *ctx = lds_ctx[wave_in_wg];
    const v4i zero = {0, 0, 0, 0};
    *reinterpret_cast<v4i *>(slab + lane * 16) = zero;
    *reinterpret_cast<v4i *>(slab + 1024 + lane * 16) = zero;
    const unsigned k = (active && cls) ? (uniform_byte(cls, r) & 3u) : 3u;
    if (lane < kEntropyCtxPerSize) ctx[lane] = init.p[k * kEntropyCtxPerSize + lane];
    if (lane == 0) lds_count[wave_in_wg] = 0;
    __syncthreads();
    if (lane == 0 && ok) {                                                  // the serial section
        EntropyDec d;
        entropy_dec_start(d, reinterpret_cast<const uint8_t *>(pay + phase), n_bytes);
        uint32_t count = 0;
        const bool good = entropy_decode_region(d, reinterpret_cast<int16_t *>(slab), k, ctx, &count);
        lds_count[wave_in_wg] = good ? count : kMalformed;
    }
    __syncthreads();
    if (!active) return;
    uint32_t count = lds_count[wave_in_wg];
    v4i a = *reinterpret_cast<const v4i *>(slab + lane * 16), b = *reinterpret_cast<const v4i *>(slab + 1024 + lane * 16);
    if (count == kMalformed) {                                              // a malformed region leaves as zeros
        a = b = zero;
        count = 0;
    }
    char *dst = reinterpret_cast<char *>(level) + r * kRegionBytes + lane * 16;
    store16<true>(dst, a);
    store16<true>(dst + 1024, b);
    if (nnz && lane == 0) nnz[r] = count;
}

EntropyInit entropy_table(const uint16_t *init)
{
    EntropyInit t = kEntropyDefault;
    if (init)
        for (unsigned i = 0; i < kEntropyContexts; ++i) t.p[i] = init[i];
    return t;
}

}  // namespace

hipError_t launch_entropy_encode(const x266_entropy_t &p, hipStream_t stream)
{
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kEntropyWavesPerWg, &wgs)) return e;
    const dim3 block(64 * kEntropyWavesPerWg);
    const EntropyInit init = entropy_table(p.init);
    if (p.n_regions) {
        hipLaunchKernelGGL(entropy_encode_kernel<false>, dim3(wgs), block, 0, stream, (const int16_t *)p.d_level, p.d_class, (const uint32_t *)p.d_nnz, p.d_region,
                           (uint16_t *)nullptr, p.n_regions, (uint64_t)0, init);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(levels_scan_kernel<x266_entropy_region_t>, dim3(1), dim3(kLevelsScanChunk), 0, stream, p.d_region, p.n_regions, p.cap_words, p.d_total);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.n_regions && p.cap_words && p.d_stream)
        hipLaunchKernelGGL(entropy_encode_kernel<true>, dim3(wgs), block, 0, stream, (const int16_t *)p.d_level, p.d_class, (const uint32_t *)p.d_nnz, p.d_region,
                           p.d_stream, p.n_regions, p.cap_words, init);
    return hipGetLastError();
}

hipError_t launch_entropy_decode(const x266_entropy_t &p, hipStream_t stream)
{
    if (p.n_regions == 0) return hipSuccess;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_regions, kEntropyWavesPerWg, &wgs)) return e;
    hipLaunchKernelGGL(entropy_decode_kernel, dim3(wgs), dim3(64 * kEntropyWavesPerWg), 0, stream, p.d_level, p.d_class, p.d_nnz,
                       (const x266_entropy_region_t *)p.d_region, (const uint16_t *)p.d_stream, p.n_regions, p.cap_words, entropy_table(p.init));
    return hipGetLastError();
}

}  // namespace x266
