// intra_kernels.hip -- 32x32 intra prediction, gfx950.
//
// The HEVC 35-mode predictor the reference's WIP RTL sketch tabulates (src/mkIntra32-wip.bsv:
// IntraRef_t :36-39, iIdx / iFact tables :75-112, projected side references :150-316, two-tap
// interpolation :358-361, DC :380-384) -- H.265 8.4.4.2.4-6 at nTbS = 32: mode 0 planar, 1 DC,
// 2..34 angular, references used as given.  PARITY UNPINNED upstream (no C model); bit-exact with
// this repository's oracle.
//
// One wave per predicted block (reference set r, mode m): 144 bytes in, 1 KiB out -- a write-bound
// byte kernel.  The wave builds the extended reference array ref[-32 .. 65] in a private LDS slot
// (main side as it lies, negative positions projected from the other side with invAngle); lane
// (k = l >> 1, h = l & 1) then interpolates 16 consecutive samples of line k: its two taps are
// adjacent bytes of ref[], so one v_dot4_u32_u8 per sample against the weights (32 - f, f) with
// the rounding term as the accumulator.  The vertical family (modes 18..34) produces rows and is
// stored directly; the horizontal family (2..17) produces columns and is turned through a 1 KiB
// LDS tile with the transposing read ds_read_b64_tr_b8.  Stores are 1 KiB-linear, "sc1 nt" (x266_device.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_device.hpp"
#include "x266_hadamard.hpp"
#include "x266_intra.hpp"
#include "x266_mfma_blocks.hpp"

namespace x266 {
namespace {

// the predictor itself (angles, predict_line16, the column turns) and the Hadamard score of a mode pair live in x266_intra.hpp: the frame
// kernels of intra_frame_kernels.hip are built on the same functions

constexpr int kUnits = 7;           // predictions per wave: one round trip fetches all seven reference sets (7 x 9 pieces of 16 bytes = 63 lanes)
constexpr int kSlotBytes = 16 + 2 * kUnits * kRawBytes + kExtBytes + 1024;   // two raw areas (current round, next round)

// A wave takes `rounds` x kUnits consecutive predictions.  Per round ONE round trip fetches the modes, the set indices and
// then all seven reference sets (7 x 9 pieces of 16 bytes, nontemporal); the NEXT round's indices and sets are fetched
// while the current round is computed (two raw areas in the wave's LDS slot), so only the first round trip of a wave is
// exposed.  (Four units per wave and no prefetch, round 1: 0.51 of the HBM peak written; seven: 0.62.)
__global__ __launch_bounds__(256) void intra32_predict_kernel(const x266_intra_ref_t *__restrict__ refs,
                                                              const uint8_t *__restrict__ modes,
                                                              const uint32_t *__restrict__ ref_index,
                                                              uint8_t *__restrict__ pred, size_t n, int rounds)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kSlotBytes];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t unit0 = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_wg) * (size_t)(kUnits * rounds);
    if (unit0 >= n) return;
    unsigned char *slot = lds + wave_in_wg * kSlotBytes;
    unsigned char *raw2 = slot + 16;                        // two raw areas; set j of area a at raw2 + a*kUnits*144 + 144 j: left[64] | top[65]
    unsigned char *ext = raw2 + 2 * kUnits * kRawBytes;     // ext[e] = ref[e - 32]
    unsigned char *tile = ext + kExtBytes;

    const int ju = lane < kUnits ? lane : kUnits - 1;
    const int set = lane / 9, piece = lane - 9 * set;       // lanes 0..62 fetch 7 x 9 pieces of 16 bytes
    auto fetch_index = [&](size_t first, int &mode_out, uint32_t &ref_out) {
        size_t u = first + ju;
        if (u >= n) u = n - 1;
        mode_out = modes[u];
        ref_out = ref_index ? ref_index[u] : (uint32_t)u;
    };
    auto fetch_sets = [&](uint32_t my_ref) -> v4i {
        const uint32_t r = (uint32_t)__shfl((int)my_ref, set < kUnits ? set : 0);
        v4i v = {0, 0, 0, 0};
        if (lane < 9 * kUnits) v = load16<true>(reinterpret_cast<const unsigned char *>(refs + r) + piece * 16);
        return v;
    };
    int my_mode, next_mode = 0;
    uint32_t my_ref, next_ref = 0;
    fetch_index(unit0, my_mode, my_ref);
    v4i sets = fetch_sets(my_ref);
    if (rounds > 1) fetch_index(unit0 + kUnits, next_mode, next_ref);
    if (lane < 9 * kUnits) *reinterpret_cast<v4i *>(raw2 + lane * 16) = sets;
    __builtin_amdgcn_wave_barrier();

#pragma unroll 1
    for (int rd = 0; rd < rounds; ++rd) {
        const size_t base = unit0 + (size_t)rd * kUnits;
        if (base >= n) break;
        const bool more = rd + 1 < rounds && base + kUnits < n;
        int mode_after = 0;
        uint32_t ref_after = 0;
        if (more) {                                          // next round's sets (and the round after's indices) in flight during this round
            sets = fetch_sets(next_ref);
            if (rd + 2 < rounds) fetch_index(base + 2 * kUnits, mode_after, ref_after);
        }
        const unsigned char *raw_all = raw2 + (rd & 1) * (kUnits * kRawBytes);
#pragma unroll 1
        for (int j = 0; j < kUnits; ++j) {
            const size_t unit = base + j;
            if (unit >= n) break;
            const int mode = __builtin_amdgcn_readlane(my_mode, j);
            const unsigned char *left = raw_all + j * kRawBytes, *top = left + 64;   // top[0] = corner
            uint32_t px[4];
            unsigned at = (unsigned)lane * 16;                       // rows: lane (k, h) holds samples 16h.. of row k
            if (predict_line16(mode, left, top, ext, lane, px)) at = turn_columns(tile, lane, px);   // columns: turned through the tile
            store16_sc1(pred + unit * 1024 + at, v4i{(int)px[0], (int)px[1], (int)px[2], (int)px[3]});
        }
        if (more) {
            if (lane < 9 * kUnits) *reinterpret_cast<v4i *>(raw2 + ((rd + 1) & 1) * (kUnits * kRawBytes) + lane * 16) = sets;
            __builtin_amdgcn_wave_barrier();
            my_mode = next_mode;
            next_mode = mode_after;
            next_ref = ref_after;
        }
    }
}

// ---- prediction -> residual -> forward DCT32 in one kernel (round 5) ------------------------------------------------------
// coef[i] = DCT32(src[i] - prediction(refs[ref_index[i]], modes[i])): the encoder loop's form of intra coding -- the chosen mode's
// prediction is consumed where it is made and never reaches HBM (1 KiB of source + 144 B of references in, 2 KiB of coefficients
// out, against 144 B + 1 KiB out for the predictor, 2 + 2 KiB + 2 KiB for residual formation and 2 + 2 KiB for the transform).
// predict_line16<true> makes the prediction directly as the A-operand fragment of the 32x32 matrix core (lane = row, 16 samples of
// half h); the horizontal family's columns are turned by the transposing LDS read addressed so that the RECEIVING lane is the
// fragment lane.  The transform is linear before its first rounding, so pass 1 is G * src + (-G) * pred on the 8-bit samples as
// they are -- one byte plane per operand, the +128 of the signed-offset trick cancels (dct32_from_tiles_kernel's scheme).
// A wave takes kFusedUnits consecutive blocks and fetches everything they need UP FRONT (modes, set indices, the sets, the source
// fragments): no loop-carried prefetch, so the compiler's own wait counts stay exact (every load is older than every store).
constexpr int fused_slot_bytes(int units) { return 16 + units * kRawBytes + kExtBytes + 1024 + 2048; }   // raw sets | ext | column tile | output converter

template <int kFusedUnits>
__global__ __launch_bounds__(256) void intra32_residual_dct32_kernel(const x266_intra_ref_t *__restrict__ refs,
                                                                     const uint8_t *__restrict__ modes,
                                                                     const uint32_t *__restrict__ ref_index,
                                                                     const uint8_t *__restrict__ src, int16_t *__restrict__ coef,
                                                                     size_t n, const DctOps *__restrict__ ops, unsigned lds_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t unit0 = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_wg) * (size_t)kFusedUnits;
    if (unit0 >= n) return;
    unsigned char *slot = lds + wave_in_wg * lds_per_wave;
    unsigned char *raw = slot + 16, *ext = raw + kFusedUnits * kRawBytes, *tile = ext + kExtBytes, *conv = tile + 1024;
    const int count = n - unit0 < (size_t)kFusedUnits ? (int)(n - unit0) : kFusedUnits;

    // everything the wave's blocks need, issued at once: modes + set indices (lanes 0..3), then the sets (4 x 9 pieces of 16 bytes)
    // and every block's source fragment (row lane & 31, bytes 16 (lane >> 5) ..: the instruction covers the block's 1 KiB whole)
    const int ju = lane < count ? lane : count - 1;
    const int my_mode = modes[unit0 + ju];
    const uint32_t my_ref = ref_index ? ref_index[unit0 + ju] : (uint32_t)(unit0 + ju);
    v4i sv[kFusedUnits];
    const unsigned char *sp = src + unit0 * 1024 + (size_t)(lane & 31) * 32 + (size_t)(lane >> 5) * 16;
#pragma unroll
    for (int j = 0; j < kFusedUnits; ++j) sv[j] = load16<true>(sp + (size_t)(j < count ? j : count - 1) * 1024);
    {
        const int set = lane / 9, piece = lane - 9 * set;
        const uint32_t r = (uint32_t)__shfl((int)my_ref, set < count ? set : 0);
        if (lane < 9 * count) *reinterpret_cast<v4i *>(raw + lane * 16) = load16<true>(reinterpret_cast<const unsigned char *>(refs + r) + piece * 16);
    }
    const LaneConsts k = load_consts(ops, lane);
    __builtin_amdgcn_wave_barrier();
    const TileLanes t = tile_lanes(lane);
#pragma unroll
    for (int j = 0; j < kFusedUnits; ++j) {
        if (j >= count) break;
        const int mode = __builtin_amdgcn_readlane(my_mode, j);
        const unsigned char *left = raw + j * kRawBytes, *top = left + 64;
        uint32_t px[4];
        if (predict_line16<true>(mode, left, top, ext, lane, px)) turn_columns_to_fragment(tile, lane, px);
        const v4i pv = {(int)px[0], (int)px[1], (int)px[2], (int)px[3]};
        v4i o0, o1, s0, s1;
        fwd_from_pixels(sv[j], pv, k, o0, o1);
        __builtin_amdgcn_wave_barrier();
        frag_to_linear(conv, t, o0, o1, s0, s1);
        char *dst = reinterpret_cast<char *>(coef) + (unit0 + j) * 2048 + lane * 16;
        store16_sc1nt(dst, s0);
        store16_sc1nt(dst + 1024, s1);
    }
}

// ---- mode decision ("Decide" channel of the RTL sketch, IntraChannel_t :41-44) ------------------
// costs[b][m] = sum over the sixteen 8x8 sub-blocks of satd8x8(src - prediction m), m = 0..34, without
// the predictions ever leaving the CU.  The Hadamard transform is linear and a 9-bit difference cannot
// wrap int16, so satd(src - pred) = (sum |H src - H pred| + 2) >> 2 per sub-block (as in me_kernels.hip):
// H src is formed once per block, H pred once per mode -- two modes per matrix-core pass, their
// 16 + 16 sub-blocks being the 32 columns of the 64x64x32 Hadamard GEMM -- and scored with v_sad_u16.
constexpr int kCostSlot = 16 + kRawBytes + kExtBytes + kTile + kTileB + kTile;   // raw | ext | src tile | two prediction tiles

__global__ __launch_bounds__(256) void intra32_costs_kernel(const x266_intra_ref_t *__restrict__ refs,
                                                            const uint8_t *__restrict__ src,
                                                            uint32_t *__restrict__ costs, uint8_t *__restrict__ best_mode,
                                                            size_t n)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kCostSlot];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t b = (size_t)blockIdx.x * (blockDim.x >> 6) + wave_in_wg;
    if (b >= n) return;
    unsigned char *raw = lds + wave_in_wg * kCostSlot + 16;
    unsigned char *ext = raw + kRawBytes, *stile = ext + kExtBytes, *ptile = stile + kTile;
    if (lane < 9) *reinterpret_cast<v4i *>(raw + lane * 16) = load16<true>(reinterpret_cast<const unsigned char *>(refs + b) + lane * 16);
    cost_stage_source(stile, lane, load16<true>(src + b * 1024 + lane * 16));
    __builtin_amdgcn_wave_barrier();
    const unsigned char *left = raw, *top = raw + 64;

    const unsigned frag = cost_window_offset(lane);
    const HadamardOps H = make_hadamard_ops(lane);
    uint32_t cs[16];
    {
        v4i w0, w1;
        cost_window(stile, frag, w0, w1);
        hadamard_pack(H, w0, w1, cs);
    }
    uint32_t best_key = 0xFFFFFFFFu;
#pragma unroll 1
    for (int pair = 0; pair < 18; ++pair) {
        const int m_a = 2 * pair, m_b = 2 * pair + 1;
        uint32_t c_a, c_b;
        intra_score_modes(m_a, m_b, m_b < 35, left, top, ext, ptile, H, cs, lane, frag, c_a, c_b);
        if (lane == 0) {
            costs[b * 35 + m_a] = c_a;
            if (m_b < 35) costs[b * 35 + m_b] = c_b;
        }
        const uint32_t k_a = (c_a << 6) | (uint32_t)m_a, k_b = m_b < 35 ? ((c_b << 6) | (uint32_t)m_b) : 0xFFFFFFFFu;
        best_key = k_a < best_key ? k_a : best_key;
        best_key = k_b < best_key ? k_b : best_key;
    }
    if (best_mode && lane == 0) best_mode[b] = (uint8_t)(best_key & 63u);
}

}  // namespace

hipError_t launch_intra32_predict(const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index,
                                  uint8_t *d_pred, size_t n, int rounds, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (rounds < 1) rounds = 1;
    while (rounds > 1 && n / (size_t)(kUnits * rounds) < 8192) --rounds;      // small batches: keep the grid large enough to fill the chip
    const size_t per_wave = (size_t)kUnits * rounds;
    unsigned wgs;
    if (hipError_t e = wave_grid((n + per_wave - 1) / per_wave, 4, &wgs)) return e;
    // (not write-bound: capping the resident waves the way the write-only stream likes it -- 10 per CU, 7.4 TB/s -- slows this
    //  kernel from 5.4 to 3.2-5.1 TB/s written; it is paced by its own VALU + LDS work, profiles/r04_intra_occupancy.txt)
    hipLaunchKernelGGL(intra32_predict_kernel, dim3(wgs), dim3(256), 0, stream, d_refs, d_modes, d_ref_index, d_pred, n, rounds);
    return hipGetLastError();
}

hipError_t launch_intra32_residual_dct32(const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index, const uint8_t *d_src,
                                         int16_t *d_coef, size_t n, const DctOps *d_fwd_ops, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    // launch shape (tools/probes/gpu_intra_fused.py over units 1 / 2 / 4 / 7 x workgroup 64 / 128 / 256 x LDS charge, profiles/r05_intra_fused.txt): everything
    // from 2 units per wave up lies within 3 %, occupancy caps only cost -- the kernel runs at what its 1 : 2 read : write mix allows
    constexpr int kUnitsPerWave = 4;
    unsigned wgs;
    if (hipError_t e = wave_grid((n + kUnitsPerWave - 1) / kUnitsPerWave, 4, &wgs)) return e;
    constexpr unsigned per_wave = (unsigned)((fused_slot_bytes(kUnitsPerWave) + 15) & ~15);
    hipLaunchKernelGGL(intra32_residual_dct32_kernel<kUnitsPerWave>, dim3(wgs), dim3(256), 4 * per_wave, stream, d_refs, d_modes, d_ref_index, d_src, d_coef, n, d_fwd_ops, per_wave);
    return hipGetLastError();
}

}  // namespace x266

namespace x266 {

hipError_t launch_intra32_costs(const x266_intra_ref_t *d_refs, const uint8_t *d_src, uint32_t *d_costs, uint8_t *d_best_mode,
                                size_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n, 4, &wgs)) return e;
    hipLaunchKernelGGL(intra32_costs_kernel, dim3(wgs), dim3(256), 0, stream, d_refs, d_src, d_costs, d_best_mode, n);
    return hipGetLastError();
}

}  // namespace x266
