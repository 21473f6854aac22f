// entropy_side_kernels.hip -- the entropy coder of the side information (xEntropyEncodeSideGpu, xEntropyDecodeSideGpu).  The contract is
// include/x266hip.h's; the canonical form, the mode lists and the syntax of a CTU are x266_entropy_side.hpp's and the coder
// x266_entropy.hpp's -- the very functions the host helpers run.
//
// The shape is not the other two coders': ONE LANE per CTU, one wave a workgroup.  A CTU has at most 161 bins; a wave with the chain on
// lane 0 would idle 63 lanes.  Each lane loads its CTU's 6 entries of each array itself, packs them into five registers (EntropySideCtu),
// and carries its own EntropyEnc / EntropyDec in registers.  What the chain indexes at run time sits in LDS, and every lane touches its
// own part of it only, so the kernels have no barrier:
//   contexts   context-major, the lane the fast index: context i of lane l is the 16-bit element at byte 4 (64 i + l).  16-bit elements,
//              because that is what entropy_enc_bin takes, at a 4-byte pitch, because LDS banks on (a / 4) % 32: whichever context each
//              lane of a 32-lane half is at, the 32 lanes hit 32 banks.  4 KB.
//   bytes      a slab of 84 bytes per lane: the 80 of the largest substream and the pad byte, 21 dwords -- an odd count, so lanes at the
//              same byte of their substreams hit different banks.  5.25 KB, only in the write step and in decode.
// The bytes cross the slab with a per-lane copy in 16-bit words: substream_copy moves one substream with a whole wave and wants slabs at
// the stream's 16-byte phase, which a 21-dword pitch does not give.  Encode is count, the level stream's offset scan on this record,
// write; decode is one launch.  Lanes diverge, bounded by the syntax.
// No atomics, no allocation, no workgroup waits for another: the bytes depend on the data alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_entropy.hpp"
#include "x266_entropy_side.hpp"
#include "x266_levels.hpp"

namespace x266 {
namespace {

constexpr unsigned kSideLanes = 64;                                         // CTUs of a workgroup
constexpr unsigned kSideCtxPitch = 2;                                       // 16-bit elements from one lane's context to the next lane's
constexpr unsigned kSideCtxStride = kSideLanes * kSideCtxPitch;            // ... and from one context to the next of the same lane
constexpr unsigned kSideSlabBytes = kEntropySideMaxBytes + 4;
static_assert(kSideSlabBytes % 4 == 0 && (kSideSlabBytes / 4) % 2 == 1, "an odd number of dwords per lane");
static_assert(sizeof(x266_entropy_side_ctu_t) == 32 && offsetof(x266_entropy_side_ctu_t, offset) == offsetof(x266_level_region_t, offset) &&
                  offsetof(x266_entropy_side_ctu_t, n_words) == offsetof(x266_level_region_t, n_words),
              "the offset scan reads n_words and writes offset where the level record has them");

struct SideArrays {
    uint8_t *kind, *mode, *cls, *qp;
    uint32_t *nnz;
};

__device__ __forceinline__ uint16_t *side_contexts(uint16_t *lds_ctx, unsigned lane, const EntropySideInit &init)
{
    uint16_t *ctx = lds_ctx + lane * kSideCtxPitch;
#pragma unroll
    for (unsigned i = 0; i < kEntropySideContexts; ++i) ctx[i * kSideCtxStride] = init.p[i];
    return ctx;
}

// WRITE false: the count step, every field of the record but `offset`.  WRITE true: the write step, after the scan.
template <bool WRITE>
__global__ __launch_bounds__(kSideLanes) void entropy_side_encode_kernel(const SideArrays in, x266_entropy_side_ctu_t *coded, uint16_t *__restrict__ stream, size_t n_ctu,
                                                                         uint64_t cap_words, int qp, int chroma_qp_offset, const EntropySideInit init)
{
    __shared__ uint16_t lds_ctx[kEntropySideContexts * kSideCtxStride];
    __shared__ __attribute__((aligned(4))) uint8_t lds_slab[WRITE ? kSideLanes * kSideSlabBytes : 4];
    const unsigned lane = threadIdx.x;
    const size_t c = (size_t)blockIdx.x * kSideLanes + lane;
    if (c >= n_ctu) return;
    uint64_t offset = 0;
    uint32_t n_words = 0;
    if (WRITE) {
        n_words = coded[c].n_words;
        offset = coded[c].offset;
        if (n_words == 0 || offset > cap_words || n_words > cap_words - offset) return;
    }
    const size_t r = 6 * c;
    const EntropySideCtu s = entropy_side_canon(in.kind ? in.kind + r : nullptr, in.mode ? in.mode + r : nullptr, in.cls ? in.cls + r : nullptr,
                                                in.qp ? in.qp + r : nullptr, in.nnz ? in.nnz + r : nullptr, qp, chroma_qp_offset);
    uint16_t *ctx = side_contexts(lds_ctx, lane, init);
    uint8_t *slab = lds_slab + (WRITE ? lane * kSideSlabBytes : 0u);
    EntropyEnc e;
    entropy_enc_start(e, WRITE ? slab : nullptr, WRITE ? kEntropySideMaxBytes : 0u);
    entropy_side_encode_ctu(e, s, ctx, kSideCtxStride, qp, chroma_qp_offset);
    const uint32_t n_bytes = entropy_enc_finish(e);
    if (!WRITE) {
        x266_entropy_side_ctu_t *rec = coded + c;
        rec->ctx_bins = e.ctx_bins;
        rec->bypass_bins = e.bypass_bins;
        rec->n_words = (n_bytes + 1u) >> 1;
        rec->n_bytes = n_bytes;
        rec->n_intra = (unsigned)__popc(s.kind);
        rec->n_coded = (unsigned)__popc(s.coded);
        return;
    }
    if (n_bytes > kEntropySideMaxBytes || ((n_bytes + 1u) >> 1) != n_words) return;        // as counted; held against the record all the same
    if (n_bytes & 1u) slab[n_bytes] = 0;                                    // the pad byte
    const uint16_t *from = reinterpret_cast<const uint16_t *>(slab);
    for (uint32_t w = 0; w < n_words; ++w) stream[offset + w] = from[w];    // at most 40 words, all below cap_words
}

__global__ __launch_bounds__(kSideLanes) void entropy_side_decode_kernel(const SideArrays out, const x266_entropy_side_ctu_t *__restrict__ coded,
                                                                         const uint16_t *__restrict__ stream, uint8_t *__restrict__ status, size_t n_ctu,
                                                                         uint64_t cap_words, int qp, int chroma_qp_offset, const EntropySideInit init)
{
    __shared__ uint16_t lds_ctx[kEntropySideContexts * kSideCtxStride];
    __shared__ __attribute__((aligned(4))) uint8_t lds_slab[kSideLanes * kSideSlabBytes];
    const unsigned lane = threadIdx.x;
    const size_t c = (size_t)blockIdx.x * kSideLanes + lane;
    if (c >= n_ctu) return;
    uint64_t offset = coded[c].offset;
    uint32_t n_bytes = coded[c].n_bytes;
    uint32_t n_words = (n_bytes >> 1) + (n_bytes & 1u);                      // no wrap at 2^32 - 1
    const bool ok = n_bytes <= kEntropySideMaxBytes && offset <= cap_words && n_words <= cap_words - offset;
    if (!ok) {                                                              // the empty substream
        offset = 0;
        n_bytes = n_words = 0;
    }
    uint8_t *slab = lds_slab + lane * kSideSlabBytes;
    uint16_t *to = reinterpret_cast<uint16_t *>(slab);
    for (uint32_t w = 0; w < n_words; ++w) to[w] = stream[offset + w];      // at most 40 words, all below cap_words
    uint16_t *ctx = side_contexts(lds_ctx, lane, init);
    EntropyDec d;
    entropy_dec_start(d, slab, n_bytes);
    EntropySideCtu s;
    uint32_t st = ok ? 0u : 1u;
    if (!entropy_side_decode_ctu(d, ctx, kSideCtxStride, qp, chroma_qp_offset, &s)) {
        s = entropy_side_flat_ctu(qp, chroma_qp_offset);
        st = 2u;
    }
    const size_t r = 6 * c;
    entropy_side_store(s, out.kind ? out.kind + r : nullptr, out.mode ? out.mode + r : nullptr, out.cls ? out.cls + r : nullptr, out.qp ? out.qp + r : nullptr,
                       out.nnz ? out.nnz + r : nullptr);
    if (status) status[c] = (uint8_t)st;
}

EntropySideInit entropy_side_table(const uint16_t *init)
{
    EntropySideInit t = kEntropySideDefault;
    if (init)
        for (unsigned i = 0; i < kEntropySideContexts; ++i) t.p[i] = init[i];
    return t;
}

SideArrays side_arrays(const x266_entropy_side_t &p) { return SideArrays{p.d_kind, p.d_mode, p.d_class, p.d_qp, p.d_nnz}; }

}  // namespace

hipError_t launch_entropy_side_encode(const x266_entropy_side_t &p, hipStream_t stream)
{
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_ctu, kSideLanes, &wgs)) return e;
    const EntropySideInit init = entropy_side_table(p.init);
    if (p.n_ctu) {
        hipLaunchKernelGGL(entropy_side_encode_kernel<false>, dim3(wgs), dim3(kSideLanes), 0, stream, side_arrays(p), p.d_coded, (uint16_t *)nullptr, p.n_ctu, (uint64_t)0,
                           p.qp, p.chroma_qp_offset, init);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(levels_scan_kernel<x266_entropy_side_ctu_t>, dim3(1), dim3(kLevelsScanChunk), 0, stream, p.d_coded, p.n_ctu, p.cap_words, p.d_total);
    if (hipError_t e = hipGetLastError()) return e;
    if (p.n_ctu && p.cap_words && p.d_stream)
        hipLaunchKernelGGL(entropy_side_encode_kernel<true>, dim3(wgs), dim3(kSideLanes), 0, stream, side_arrays(p), p.d_coded, p.d_stream, p.n_ctu, p.cap_words, p.qp,
                           p.chroma_qp_offset, init);
    return hipGetLastError();
}

hipError_t launch_entropy_side_decode(const x266_entropy_side_t &p, hipStream_t stream)
{
    if (p.n_ctu == 0) return hipSuccess;
    unsigned wgs = 0;
    if (hipError_t e = wave_grid(p.n_ctu, kSideLanes, &wgs)) return e;
    hipLaunchKernelGGL(entropy_side_decode_kernel, dim3(wgs), dim3(kSideLanes), 0, stream, side_arrays(p), (const x266_entropy_side_ctu_t *)p.d_coded,
                       (const uint16_t *)p.d_stream, p.d_status, p.n_ctu, p.cap_words, p.qp, p.chroma_qp_offset, entropy_side_table(p.init));
    return hipGetLastError();
}

}  // namespace x266
