// intra_frame_kernels.hip -- 32x32 intra coding of a whole tiled frame (include/x266hip.h: xIntra32RefsFromTilesGpu,
// xIntra32CodeFrameGpu), gfx950.  Composed from the blocks the library already has: the 35-mode predictor and the Hadamard score of
// x266_intra.hpp, code_region of x266_code_region.hpp (forward DCT32, quantise, dequantise, inverse), the tile addressing of
// x266_ctu_tiles.hpp.
//
// The reference set of a block is gathered from a tiled frame sample by sample: 129 samples in the order left[63] .. left[0],
// top[0] .. top[64], in five segments (BL, L, C, T, TR) that are available or not as a whole; an unavailable sample takes the value
// of the last available one before it, in front of the first available one that one's value, 128 when there is none (gather_set).
//
// intra32_refs_from_tiles_kernel is the open-loop form: one wave per set, the sets of a frame's own samples, fully parallel.
//
// intra_frame_step_kernel is one step of the closed loop, in which a block's references are the RECONSTRUCTED samples of its
// neighbours.  Region (cx, cy, q) runs at step T = 4 cx + 6 cy + q and a CTU's chroma at its q = 3 step: every segment the header's
// rule makes available was written at an earlier step (left: T - 1 or T - 3, above: T - 2 or T - 4, above right: T - 1 .. T - 3,
// below left of q = 0: T - 1; chroma left T - 4, above T - 6, above right T - 2), so the order of the launches on the stream is the
// only synchronisation: no workgroup waits for another.  A step has at most one luma block and one chroma pair per CTU row and is
// latency-bound, so a block gets a whole workgroup: its four waves score a share of the 18 mode pairs each and reduce
// (cost << 6 | mode) keys through LDS, then wave 0 predicts in fragment lanes and codes the region.  With the modes given the
// workgroup is that one wave.
//
// mixed_inter_regions_kernel and mixed_frame_step_kernel (xDct32CodeMixedFrameGpu) code a frame whose regions are inter or intra, region
// by region, from the same pieces on the same schedule: see "mixed inter / intra coding of a frame" below.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x266_code_region.hpp"
#include "x266_ctu_tiles.hpp"
#include "x266_device.hpp"
#include "x266_hadamard.hpp"
#include "x266_intra.hpp"
#include "x266_mfma_blocks.hpp"
#include "x266_quant.hpp"
#include "x266_tables.hpp"

namespace x266 {
namespace {

// byte offset of sample (x, y) of component comp (0 = Y in m_Y, 1 = U and 2 = V in the interleaved m_C; x, y on that component's grid)
__device__ __forceinline__ size_t sample_offset(int comp, int x, int y, int tiles_x)
{
    if (comp == 0) return ((size_t)(y >> 4) * (size_t)tiles_x + (size_t)(x >> 4)) * sizeof(x266_ref_block_t) + (size_t)((y & 15) * 16 + (x & 15));
    return ((size_t)(y >> 3) * (size_t)tiles_x + (size_t)(x >> 3)) * sizeof(x266_ref_block_t) + (size_t)(256 + (y & 7) * 16 + (x & 7) * 2 + (comp - 1));
}

// segments in scan order and their availability bits
constexpr unsigned kSegBL = 1u, kSegL = 2u, kSegC = 4u, kSegT = 8u, kSegTR = 16u;

// luma block (bx, by) of a frame of blocks_x x blocks_y 32x32 blocks; quadrant q = 2 (by & 1) + (bx & 1) of its CTU
__device__ __forceinline__ unsigned luma_availability(int bx, int by, int blocks_x, int blocks_y)
{
    const int q = 2 * (by & 1) + (bx & 1);
    unsigned a = 0;
    if (bx > 0) a |= kSegL;
    if (by > 0) a |= kSegT;
    if (bx > 0 && by > 0) a |= kSegC;
    if (by > 0 && bx + 1 < blocks_x && q != 3) a |= kSegTR;
    if (bx > 0 && by + 1 < blocks_y && q == 0) a |= kSegBL;
    return a;
}
// the 32x32 U or V block of CTU (cx, cy)
__device__ __forceinline__ unsigned chroma_availability(int cx, int cy, int ctus_x)
{
    unsigned a = 0;
    if (cx > 0) a |= kSegL;
    if (cy > 0) a |= kSegT;
    if (cx > 0 && cy > 0) a |= kSegC;
    if (cy > 0 && cx + 1 < ctus_x) a |= kSegTR;
    return a;
}

// One wave builds the set of the 32x32 block whose top-left sample is (x0, y0) of component comp in raw[0 .. 143]: left[64] | top[65] |
// 15 zero bytes.  Only samples of available segments are read, and those lie inside the frame.  `avail` is wave-uniform.
__device__ __forceinline__ void gather_set(const unsigned char *frame, int comp, int x0, int y0, int tiles_x, unsigned avail, unsigned char *raw, int lane)
{
    // scan index i = 0 .. 128 -> its place in raw: left[63 - i] for i < 64, top[i - 64] behind the 64 left bytes
    auto place = [](int i) { return i < 64 ? 63 - i : i; };
    auto segment = [](int i) { return i < 32 ? 0 : i < 64 ? 1 : i == 64 ? 2 : i < 97 ? 3 : 4; };
#pragma unroll
    for (int rep = 0; rep < 3; ++rep) {
        const int i = lane + 64 * rep;
        if (i < 129 && ((avail >> segment(i)) & 1u)) {
            const int x = i < 64 ? x0 - 1 : x0 + i - 65, y = i < 64 ? y0 + 63 - i : y0 - 1;
            raw[place(i)] = frame[sample_offset(comp, x, y, tiles_x)];
        }
    }
    if (lane < 15) raw[129 + lane] = 0;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int rep = 0; rep < 3; ++rep) {
        const int i = lane + 64 * rep;
        if (i < 129) {
            const int s = segment(i);
            if (!((avail >> s) & 1u)) {
                const unsigned before = avail & ((1u << s) - 1u), after = avail >> (s + 1);
                unsigned v = 128;
                if (before) {                               // the last sample of the nearest available segment in front
                    const int p = 31 - __builtin_clz(before);
                    v = raw[place(p == 0 ? 31 : p == 1 ? 63 : p == 2 ? 64 : 96)];
                } else if (after) {                         // nothing in front: the first available sample of the scan
                    const int n = s + 1 + __builtin_ctz(after);
                    v = raw[place(n == 1 ? 32 : n == 2 ? 64 : n == 3 ? 65 : 97)];
                }
                raw[place(i)] = (unsigned char)v;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// ---- the open-loop gather ----------------------------------------------------------------------------------------------------------
// component 0: set 4 ctu + q; 1 / 2: set ctu.  One wave per set, four to a workgroup.
__global__ __launch_bounds__(256) void intra32_refs_from_tiles_kernel(const x266_ref_block_t *__restrict__ frame, x266_intra_ref_t *__restrict__ refs,
                                                                      int component, int ctus_x, int ctus_y, size_t n_sets)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kRawBytes];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t set = (size_t)blockIdx.x * 4 + (size_t)wave_in_wg;
    if (set >= n_sets) return;
    unsigned char *raw = lds + wave_in_wg * kRawBytes;
    const size_t ctu = component == 0 ? set >> 2 : set;
    const int cy = (int)(ctu / (size_t)ctus_x), cx = (int)(ctu - (size_t)cy * (size_t)ctus_x);
    const int tiles_x = ctus_x * 4;
    const unsigned char *base = reinterpret_cast<const unsigned char *>(frame);
    if (component == 0) {
        const int q = (int)(set & 3), bx = 2 * cx + (q & 1), by = 2 * cy + (q >> 1);
        gather_set(base, 0, 32 * bx, 32 * by, tiles_x, luma_availability(bx, by, 2 * ctus_x, 2 * ctus_y), raw, lane);
    } else {
        gather_set(base, component, 32 * cx, 32 * cy, tiles_x, chroma_availability(cx, cy, ctus_x), raw, lane);
    }
    if (lane < 9) *reinterpret_cast<v4i *>(reinterpret_cast<unsigned char *>(refs + set) + lane * 16) = *reinterpret_cast<const v4i *>(raw + lane * 16);
}

// ---- one step of the closed loop -----------------------------------------------------------------------------------------------------
// A wave's LDS: two raw sets (luma uses the first; chroma U and V) | ext | two source tiles (U, V) | two prediction tiles; the
// workgroup's 2 KiB level converter and its four keys follow the waves' slots.
constexpr int kFrameSlot = 16 + 2 * kRawBytes + kExtBytes + 2 * kTile + kTileB + kTile;
static_assert(kFrameSlot % 16 == 0 && kRawBytes % 16 == 0 && kExtBytes % 16 == 0 && kTile % 16 == 0 && kTileB % 16 == 0, "16-byte LDS pieces");
constexpr int kChromaCandidates = 5;

struct WaveSlot {
    unsigned char *raw_a, *raw_b, *ext, *stile_a, *stile_b, *ptile;
};
__device__ __forceinline__ WaveSlot wave_slot(unsigned char *lds, int wave_in_wg)
{
    WaveSlot s;
    s.raw_a = lds + wave_in_wg * kFrameSlot + 16;
    s.raw_b = s.raw_a + kRawBytes;
    s.ext = s.raw_b + kRawBytes;
    s.stile_a = s.ext + kExtBytes;
    s.stile_b = s.stile_a + kTile;
    s.ptile = s.stile_b + kTile;
    return s;
}

// the prediction of `mode` on the set at raw, as the A-operand fragment: row lane & 31, columns 16 (lane >> 5) ..
__device__ __forceinline__ v4i predict_fragment(int mode, const unsigned char *raw, unsigned char *ext, unsigned char *tile, int lane)
{
    uint32_t px[4];
    if (predict_line16<true>(mode, raw, raw + 64, ext, lane, px)) turn_columns_to_fragment(tile, lane, px);
    return v4i{(int)px[0], (int)px[1], (int)px[2], (int)px[3]};
}

// two planes' 16 samples each -> the two m_C rows (8 interleaved U,V pairs each) that hold them
__device__ __forceinline__ void interleave_chroma(const v4i &u, const v4i &v, v4i &c0, v4i &c1)
{
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        c0[2 * j] = (int)bperm((uint32_t)v[j], (uint32_t)u[j], 0x05010400u);
        c0[2 * j + 1] = (int)bperm((uint32_t)v[j], (uint32_t)u[j], 0x07030602u);
        c1[2 * j] = (int)bperm((uint32_t)v[2 + j], (uint32_t)u[2 + j], 0x05010400u);
        c1[2 * j + 1] = (int)bperm((uint32_t)v[2 + j], (uint32_t)u[2 + j], 0x07030602u);
    }
}

// grid (rows of the step, 2): y = 0 the luma block of CTU row cy_first + x at this step, y = 1 that CTU's chroma when the block is quadrant 3.
// DECIDE: four waves and the mode decision; otherwise one wave and the modes of mode_in.  mode_out may be mode_in (each workgroup reads
// its entries before it writes them, and no other workgroup touches them).
template <bool DECIDE>
__global__ __launch_bounds__(DECIDE ? 256 : 64) void intra_frame_step_kernel(const x266_ref_block_t *__restrict__ cur, x266_ref_block_t *recon,
                                                                             int16_t *__restrict__ level, uint32_t *__restrict__ nnz,
                                                                             const uint8_t *__restrict__ qps, unsigned qp, unsigned rounding,
                                                                             const uint8_t *mode_in, uint8_t *mode_out, int ctus_x, int ctus_y,
                                                                             int step, int cy_first, const DctOps *__restrict__ fwd_ops,
                                                                             const DctOps *__restrict__ inv_ops)
{
    constexpr int kWaves = DECIDE ? 4 : 1;
    __shared__ __attribute__((aligned(16))) unsigned char lds[kWaves * kFrameSlot + 2048 + 16];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cy = cy_first + (int)blockIdx.x;
    const int r = step - 6 * cy, cx = r >> 2, q = r & 3;                  // the launcher's row range keeps 0 <= cx < ctus_x
    const bool chroma = blockIdx.y != 0;
    if (chroma && q != 3) return;
    const int tiles_x = ctus_x * 4;
    const size_t ctu = (size_t)cy * (size_t)ctus_x + (size_t)cx;
    const WaveSlot s = wave_slot(lds, wave_in_wg);
    unsigned char *conv = lds + kWaves * kFrameSlot;
    uint32_t *keys = reinterpret_cast<uint32_t *>(conv + 2048);
    const unsigned char *rec = reinterpret_cast<const unsigned char *>(recon), *src = reinterpret_cast<const unsigned char *>(cur);
    const unsigned c = (unsigned)lane & 31u, h = (unsigned)lane >> 5;
    char *dst = reinterpret_cast<char *>(level + ctu * 6144) + lane * 16;
    uint32_t *cnt = nnz ? nnz + ctu * 6 : nullptr;
    // what the coding wave needs besides the mode is fetched in front of the decision, whose latency covers it
    const LaneConsts kf = load_consts(fwd_ops, lane), ki = load_consts(inv_ops, lane);
    const v16i c2r = load_c2r(inv_ops, (int)h);
    const TileLanes t = tile_lanes(lane);

    if (!chroma) {
        const int bx = 2 * cx + (q & 1), by = 2 * cy + (q >> 1);
        gather_set(rec, 0, 32 * bx, 32 * by, tiles_x, luma_availability(bx, by, 2 * ctus_x, 2 * ctus_y), s.raw_a, lane);
        int mode;
        if (DECIDE) {
            // the source block in score lanes: row lane >> 1, columns 16 (lane & 1) .. = one m_Y row of one tile
            const size_t at = sample_offset(0, 32 * bx + 16 * (lane & 1), 32 * by + (lane >> 1), tiles_x);
            cost_stage_source(s.stile_a, lane, load16<true>(src + at));
            __builtin_amdgcn_wave_barrier();
            const unsigned frag = cost_window_offset(lane);
            const HadamardOps H = make_hadamard_ops(lane);
            uint32_t cs[16];
            {
                v4i w0, w1;
                cost_window(s.stile_a, frag, w0, w1);
                hadamard_pack(H, w0, w1, cs);
            }
            uint32_t best_key = 0xFFFFFFFFu;
#pragma unroll 1
            for (int pair = wave_in_wg; pair < 18; pair += kWaves) {
                const int m_a = 2 * pair, m_b = 2 * pair + 1;
                uint32_t c_a, c_b;
                intra_score_modes(m_a, m_b, m_b < 35, s.raw_a, s.raw_a + 64, s.ext, s.ptile, H, cs, lane, frag, c_a, c_b);
                const uint32_t k_a = (c_a << 6) | (uint32_t)m_a, k_b = m_b < 35 ? ((c_b << 6) | (uint32_t)m_b) : 0xFFFFFFFFu;
                best_key = k_a < best_key ? k_a : best_key;
                best_key = k_b < best_key ? k_b : best_key;
            }
            if (lane == 0) keys[wave_in_wg] = best_key;
            __syncthreads();
            if (wave_in_wg != 0) return;
            uint32_t k = keys[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) k = keys[w] < k ? keys[w] : k;
            mode = __builtin_amdgcn_readfirstlane((int)(k & 63u));
        } else {
            mode = (int)uniform_byte(mode_in, ctu * 6 + (size_t)q);
        }
        const size_t off = ctu_luma_tile((size_t)cy, (size_t)cx, (unsigned)q, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
        const v4i a = load16<true>(src + off);
        const QuantParams qn = region_quant(qps, ctu * 6 + (size_t)q, qp, rounding);
        if (lane == 0) mode_out[ctu * 6 + (size_t)q] = (uint8_t)mode;
        const v4i b = predict_fragment(mode, s.raw_a, s.ext, s.ptile, lane);
        v4i o0, o1;
        code_region(a, b, kf, ki, c2r, qn, (unsigned)lane, conv, t, dst + q * 2048, cnt ? cnt + q : nullptr, o0, o1);
        store16_sc1nt(reinterpret_cast<unsigned char *>(recon) + off, recon_luma16(b, o0, o1));
        return;
    }

    // U and V of the CTU: one mode for both planes
    const unsigned avail = chroma_availability(cx, cy, ctus_x);
    gather_set(rec, 1, 32 * cx, 32 * cy, tiles_x, avail, s.raw_a, lane);
    gather_set(rec, 2, 32 * cx, 32 * cy, tiles_x, avail, s.raw_b, lane);
    int mode;
    if (DECIDE) {
        // score lanes: chroma row lane >> 1, columns 16 (lane & 1) .. = the m_C rows of two neighbouring tiles
        const size_t at = ctu_chroma_tile((size_t)cy, (size_t)cx, (unsigned)lane >> 1, (unsigned)lane & 1u, tiles_x) * sizeof(x266_ref_block_t) +
                          ctu_chroma_row_offset((unsigned)lane >> 1);
        const v4i a0 = load16<true>(src + at), a1 = load16<true>(src + at + 512);
        const int dm = (int)mode_out[ctu * 6];                             // quadrant 0's mode, written three steps ago
        cost_stage_source(s.stile_a, lane, chroma_plane(a0, a1, kSelU));
        cost_stage_source(s.stile_b, lane, chroma_plane(a0, a1, kSelV));
        __builtin_amdgcn_wave_barrier();
        const unsigned frag = cost_window_offset(lane);
        const HadamardOps H = make_hadamard_ops(lane);
        const int dm_u = __builtin_amdgcn_readfirstlane(dm);
        // candidates (0, 26, 10, 1, quadrant 0's mode): wave w scores positions 2w and 2w + 1; the key carries the position, so the first wins ties
        uint32_t best_key = 0xFFFFFFFFu;
        if (2 * wave_in_wg < kChromaCandidates) {
            const int m_a = wave_in_wg == 0 ? 0 : wave_in_wg == 1 ? 10 : dm_u, m_b = wave_in_wg == 0 ? 26 : 1;
            const bool have_b = 2 * wave_in_wg + 1 < kChromaCandidates;
            uint32_t cost_a = 0, cost_b = 0;
#pragma unroll 1
            for (int plane = 0; plane < 2; ++plane) {
                const unsigned char *raw = plane ? s.raw_b : s.raw_a;
                uint32_t cs[16];
                v4i w0, w1;
                cost_window(plane ? s.stile_b : s.stile_a, frag, w0, w1);
                hadamard_pack(H, w0, w1, cs);
                uint32_t c_a, c_b;
                intra_score_modes(m_a, m_b, have_b, raw, raw + 64, s.ext, s.ptile, H, cs, lane, frag, c_a, c_b);
                cost_a += c_a;
                cost_b += c_b;
            }
            best_key = (cost_a << 6) | (uint32_t)(2 * wave_in_wg);
            const uint32_t k_b = have_b ? ((cost_b << 6) | (uint32_t)(2 * wave_in_wg + 1)) : 0xFFFFFFFFu;
            best_key = k_b < best_key ? k_b : best_key;
        }
        if (lane == 0) keys[wave_in_wg] = best_key;
        __syncthreads();
        if (wave_in_wg != 0) return;
        uint32_t k = keys[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) k = keys[w] < k ? keys[w] : k;
        const int pos = __builtin_amdgcn_readfirstlane((int)(k & 63u));
        mode = pos == 0 ? 0 : pos == 1 ? 26 : pos == 2 ? 10 : pos == 3 ? 1 : dm_u;
    } else {
        mode = (int)uniform_byte(mode_in, ctu * 6 + 4);
    }
    const size_t off = ctu_chroma_tile((size_t)cy, (size_t)cx, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
    const v4i a0 = load16<true>(src + off), a1 = load16<true>(src + off + 512);        // tiles 2h and 2h + 1
    const QuantParams qu = region_quant(qps, ctu * 6 + 4, qp, rounding), qv = region_quant(qps, ctu * 6 + 5, qp, rounding);
    if (lane == 0) {
        mode_out[ctu * 6 + 4] = (uint8_t)mode;
        mode_out[ctu * 6 + 5] = (uint8_t)mode;
    }
    const v4i bu = predict_fragment(mode, s.raw_a, s.ext, s.ptile, lane);
    v4i ou0, ou1, ov0, ov1;
    code_region(chroma_plane(a0, a1, kSelU), bu, kf, ki, c2r, qu, (unsigned)lane, conv, t, dst + 4 * 2048, cnt ? cnt + 4 : nullptr, ou0, ou1);
    __builtin_amdgcn_wave_barrier();                                       // the U levels have left the converter, the U columns the tile
    const v4i bv = predict_fragment(mode, s.raw_b, s.ext, s.ptile, lane);
    code_region(chroma_plane(a0, a1, kSelV), bv, kf, ki, c2r, qv, (unsigned)lane, conv, t, dst + 5 * 2048, cnt ? cnt + 5 : nullptr, ov0, ov1);
    v4i r0, r1;
    interleave_chroma(recon_luma16(bu, ou0, ou1), recon_luma16(bv, ov0, ov1), r0, r1);
    unsigned char *pr = reinterpret_cast<unsigned char *>(recon) + off;
    store16_sc1nt(pr, r0);
    store16_sc1nt(pr + 512, r1);
}

// ---- mixed inter / intra coding of a frame (include/x266hip.h: xDct32CodeMixedFrameGpu) ---------------------------------------------------
// Every region has a kind: 0 = inter (pred comes from the motion-compensated frame), 1 = intra, 2 = the call decides by comparing the
// two predictions' Hadamard costs.  The regions given as inter depend on nothing, so ONE launch codes them all up front
// (mixed_inter_regions_kernel: the work of dct32_code_ctu_tiles_kernel with a per-region skip).  The others follow on the wavefront of
// the intra frame above, one launch per step (mixed_frame_step_kernel); a workgroup whose region was given as inter returns after reading
// its kind byte.  Stream order is the only synchronisation here too.  The inter prediction is scored through the same pieces as the
// intra modes: staged like a source tile (cost_stage_source) and scored by score_tiles, in the DECIDE form by the wave with the fewest
// mode pairs (the last one), which posts the cost next to the four keys.
struct MixedArgs {
    const x266_ref_block_t *cur, *pred;
    x266_ref_block_t *recon;
    int16_t *level;
    uint32_t *nnz;
    const uint8_t *qps, *kind_in, *mode_in;
    uint8_t *kind, *mode;
    uint32_t *cost;
    unsigned qp, rounding, penalty;
    int ctus_x, ctus_y;
    const DctOps *fwd_ops, *inv_ops;
};
constexpr uint32_t kNoCost = 0xFFFFFFFFu;
constexpr unsigned kInterMode = 255;

// what a region ended as, from lane 0 of its coding wave: `n` entries from `region` on (2 for chroma) get the same bytes and costs
__device__ __forceinline__ void mixed_region_outputs(const MixedArgs &a, size_t region, int n, unsigned kind, unsigned mode, uint32_t inter_cost, uint32_t intra_cost)
{
    for (int i = 0; i < n; ++i) {
        a.kind[region + i] = (uint8_t)kind;
        a.mode[region + i] = (uint8_t)mode;
        if (a.cost) {
            a.cost[2 * (region + i)] = inter_cost;
            a.cost[2 * (region + i) + 1] = intra_cost;
        }
    }
}

// phase 1: five waves per CTU (Y0 .. Y3, U and V together) as in dct32_code_ctu_tiles_kernel; a wave whose kind byte is not 0 returns
__global__ __launch_bounds__(256) void mixed_inter_regions_kernel(MixedArgs a, size_t n_ctus)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * 2048];
    const unsigned lane = threadIdx.x & 63;
    const unsigned wave_in_wg = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t unit = (size_t)blockIdx.x * 4 + wave_in_wg;
    const size_t ctu = unit / 5;
    const unsigned part = (unsigned)(unit - ctu * 5);
    if (ctu >= n_ctus) return;
    const size_t region = ctu * 6 + part;                                   // part 4: the chroma pair, entry 4
    if (uniform_byte(a.kind_in, region) != 0) return;
    unsigned char *slot = lds + wave_in_wg * 2048;
    const unsigned c = lane & 31, h = lane >> 5;
    const int tiles_x = a.ctus_x * 4;
    const size_t cy = ctu / (size_t)a.ctus_x, cx = ctu - cy * (size_t)a.ctus_x;
    const LaneConsts kf = load_consts(a.fwd_ops, (int)lane), ki = load_consts(a.inv_ops, (int)lane);
    const v16i c2r = load_c2r(a.inv_ops, (int)h);
    const TileLanes t = tile_lanes((int)lane);
    char *dst = reinterpret_cast<char *>(a.level + ctu * 6144) + lane * 16;
    uint32_t *cnt = a.nnz ? a.nnz + ctu * 6 : nullptr;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(a.cur), *prd = reinterpret_cast<const unsigned char *>(a.pred);
    if (part < 4) {
        const size_t off = ctu_luma_tile(cy, cx, part, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
        const v4i s = load16<true>(src + off), b = load16<true>(prd + off);
        v4i o0, o1;
        code_region(s, b, kf, ki, c2r, region_quant(a.qps, region, a.qp, a.rounding), lane, slot, t, dst + part * 2048, cnt ? cnt + part : nullptr, o0, o1);
        store16_sc1nt(reinterpret_cast<unsigned char *>(a.recon) + off, recon_luma16(b, o0, o1));
        if (lane == 0) mixed_region_outputs(a, region, 1, 0, kInterMode, kNoCost, kNoCost);
        return;
    }
    const size_t off = ctu_chroma_tile(cy, cx, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
    const v4i a0 = load16<true>(src + off), a1 = load16<true>(src + off + 512), b0 = load16<true>(prd + off), b1 = load16<true>(prd + off + 512);
    const QuantParams qu = region_quant(a.qps, region, a.qp, a.rounding), qv = region_quant(a.qps, region + 1, a.qp, a.rounding);
    v4i ou0, ou1, ov0, ov1;
    code_region(chroma_plane(a0, a1, kSelU), chroma_plane(b0, b1, kSelU), kf, ki, c2r, qu, lane, slot, t, dst + 4 * 2048, cnt ? cnt + 4 : nullptr, ou0, ou1);
    __builtin_amdgcn_wave_barrier();                                       // the U levels have left the slot
    code_region(chroma_plane(a0, a1, kSelV), chroma_plane(b0, b1, kSelV), kf, ki, c2r, qv, lane, slot, t, dst + 5 * 2048, cnt ? cnt + 5 : nullptr, ov0, ov1);
    unsigned char *pr = reinterpret_cast<unsigned char *>(a.recon) + off;
    store16_sc1nt(pr, recon_chroma16(b0, ou0, ov0));
    store16_sc1nt(pr + 512, recon_chroma16(b1, ou1, ov1));
    if (lane == 0) mixed_region_outputs(a, region, 2, 0, kInterMode, kNoCost, kNoCost);
}

// phase 2, one step: the grid of intra_frame_step_kernel.  DECIDE (mode_in == NULL): four waves and the mode decision; otherwise one wave
// and the mode of mode_in, scored only where the kind is to be decided.  kind may be kind_in and mode may be mode_in: a workgroup reads
// its own entries before it writes them and no other workgroup touches them; quadrant 0's entries, which the chroma reads, were
// written three steps ago or by phase 1.  recon may be pred: the inter prediction is read (by the scoring wave in front of the
// workgroup barrier, by the coding wave as its pred fragment) before the coding wave stores the same bytes.
template <bool DECIDE>
__global__ __launch_bounds__(DECIDE ? 256 : 64) void mixed_frame_step_kernel(MixedArgs a, int step, int cy_first)
{
    constexpr int kWaves = DECIDE ? 4 : 1;
    __shared__ __attribute__((aligned(16))) unsigned char lds[kWaves * kFrameSlot + 2048 + 32];
    const int lane = threadIdx.x & 63;
    const int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cy = cy_first + (int)blockIdx.x;
    const int r = step - 6 * cy, cx = r >> 2, q = r & 3;                  // the launcher's row range keeps 0 <= cx < ctus_x
    const bool chroma = blockIdx.y != 0;
    if (chroma && q != 3) return;
    const int ctus_x = a.ctus_x, tiles_x = ctus_x * 4;
    const size_t ctu = (size_t)cy * (size_t)ctus_x + (size_t)cx;
    const size_t region = ctu * 6 + (size_t)(chroma ? 4 : q);
    unsigned k = a.kind_in ? uniform_byte(a.kind_in, region) : 2u;
    k = k < 2u ? k : 2u;
    if (k == 0) return;                                                    // coded by phase 1
    const WaveSlot s = wave_slot(lds, wave_in_wg);
    unsigned char *conv = lds + kWaves * kFrameSlot;
    uint32_t *keys = reinterpret_cast<uint32_t *>(conv + 2048);           // four keys and the inter cost
    const unsigned char *rec = reinterpret_cast<const unsigned char *>(a.recon), *src = reinterpret_cast<const unsigned char *>(a.cur);
    const unsigned char *prd = reinterpret_cast<const unsigned char *>(a.pred);
    const unsigned c = (unsigned)lane & 31u, h = (unsigned)lane >> 5;
    char *dst = reinterpret_cast<char *>(a.level + ctu * 6144) + lane * 16;
    uint32_t *cnt = a.nnz ? a.nnz + ctu * 6 : nullptr;
    const LaneConsts kf = load_consts(a.fwd_ops, lane), ki = load_consts(a.inv_ops, lane);
    const v16i c2r = load_c2r(a.inv_ops, (int)h);
    const TileLanes t = tile_lanes(lane);
    const bool scores_inter = k == 2 && wave_in_wg == kWaves - 1;
    uint32_t inter_cost = kNoCost, intra_cost = kNoCost;

    if (!chroma) {
        const int bx = 2 * cx + (q & 1), by = 2 * cy + (q >> 1);
        gather_set(rec, 0, 32 * bx, 32 * by, tiles_x, luma_availability(bx, by, 2 * ctus_x, 2 * a.ctus_y), s.raw_a, lane);
        int mode = DECIDE ? 0 : (int)uniform_byte(a.mode_in, region);
        if (DECIDE || k == 2) {
            // source and inter prediction in score lanes: row lane >> 1, columns 16 (lane & 1) .. = one m_Y row of one tile
            const size_t at = sample_offset(0, 32 * bx + 16 * (lane & 1), 32 * by + (lane >> 1), tiles_x);
            cost_stage_source(s.stile_a, lane, load16<true>(src + at));
            if (scores_inter) cost_stage_source(s.ptile, lane, load16<true>(prd + at));
            __builtin_amdgcn_wave_barrier();
            const unsigned frag = cost_window_offset(lane);
            const HadamardOps H = make_hadamard_ops(lane);
            uint32_t cs[16];
            {
                v4i w0, w1;
                cost_window(s.stile_a, frag, w0, w1);
                hadamard_pack(H, w0, w1, cs);
            }
            uint32_t unused;
            if (scores_inter) score_tiles(s.ptile, H, cs, lane, frag, inter_cost, unused);   // the second tile holds nothing
            if (DECIDE) {
                uint32_t best_key = 0xFFFFFFFFu;
#pragma unroll 1
                for (int pair = wave_in_wg; pair < 18; pair += kWaves) {
                    const int m_a = 2 * pair, m_b = 2 * pair + 1;
                    uint32_t c_a, c_b;
                    intra_score_modes(m_a, m_b, m_b < 35, s.raw_a, s.raw_a + 64, s.ext, s.ptile, H, cs, lane, frag, c_a, c_b);
                    const uint32_t k_a = (c_a << 6) | (uint32_t)m_a, k_b = m_b < 35 ? ((c_b << 6) | (uint32_t)m_b) : 0xFFFFFFFFu;
                    best_key = k_a < best_key ? k_a : best_key;
                    best_key = k_b < best_key ? k_b : best_key;
                }
                if (lane == 0) {
                    keys[wave_in_wg] = best_key;
                    if (scores_inter) keys[4] = inter_cost;
                }
                __syncthreads();
                if (wave_in_wg != 0) return;
                uint32_t key = keys[0];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) key = keys[w] < key ? keys[w] : key;
                key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
                mode = (int)(key & 63u);
                intra_cost = key >> 6;
                if (k == 2) inter_cost = (uint32_t)__builtin_amdgcn_readfirstlane((int)keys[4]);
            } else {
                intra_score_modes(mode, mode, false, s.raw_a, s.raw_a + 64, s.ext, s.ptile, H, cs, lane, frag, intra_cost, unused);
            }
        }
        const bool intra = k == 1 || intra_cost + a.penalty < inter_cost;   // k == 2: a tie is inter; no sum reaches 2^32 (costs below 2^26)
        const size_t off = ctu_luma_tile((size_t)cy, (size_t)cx, (unsigned)q, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_luma_row_offset(c);
        const v4i sa = load16<true>(src + off);
        const QuantParams qn = region_quant(a.qps, region, a.qp, a.rounding);
        if (lane == 0) mixed_region_outputs(a, region, 1, intra ? 1u : 0u, intra ? (unsigned)mode : kInterMode, inter_cost, intra_cost);
        v4i b;
        if (intra) b = predict_fragment(mode, s.raw_a, s.ext, s.ptile, lane);
        else b = load16<true>(prd + off);
        v4i o0, o1;
        code_region(sa, b, kf, ki, c2r, qn, (unsigned)lane, conv, t, dst + q * 2048, cnt ? cnt + q : nullptr, o0, o1);
        store16_sc1nt(reinterpret_cast<unsigned char *>(a.recon) + off, recon_luma16(b, o0, o1));
        return;
    }

    // U and V of the CTU: one kind and one mode for both planes
    const unsigned avail = chroma_availability(cx, cy, ctus_x);
    gather_set(rec, 1, 32 * cx, 32 * cy, tiles_x, avail, s.raw_a, lane);
    gather_set(rec, 2, 32 * cx, 32 * cy, tiles_x, avail, s.raw_b, lane);
    int mode = DECIDE ? 0 : (int)uniform_byte(a.mode_in, region);
    if (DECIDE || k == 2) {
        // score lanes: chroma row lane >> 1, columns 16 (lane & 1) .. = the m_C rows of two neighbouring tiles
        const size_t at = ctu_chroma_tile((size_t)cy, (size_t)cx, (unsigned)lane >> 1, (unsigned)lane & 1u, tiles_x) * sizeof(x266_ref_block_t) +
                          ctu_chroma_row_offset((unsigned)lane >> 1);
        const v4i a0 = load16<true>(src + at), a1 = load16<true>(src + at + 512);
        // quadrant 0's kind and mode: its mode is a candidate only if it ended intra
        const int q0_intra = __builtin_amdgcn_readfirstlane((int)a.kind[ctu * 6]), dm_u = __builtin_amdgcn_readfirstlane((int)a.mode[ctu * 6]);
        cost_stage_source(s.stile_a, lane, chroma_plane(a0, a1, kSelU));
        cost_stage_source(s.stile_b, lane, chroma_plane(a0, a1, kSelV));
        if (scores_inter) {
            const v4i p0 = load16<true>(prd + at), p1 = load16<true>(prd + at + 512);
            cost_stage_source(s.ptile, lane, chroma_plane(p0, p1, kSelU));
            cost_stage_source(s.ptile + kTileB, lane, chroma_plane(p0, p1, kSelV));
        }
        __builtin_amdgcn_wave_barrier();
        const unsigned frag = cost_window_offset(lane);
        const HadamardOps H = make_hadamard_ops(lane);
        if (scores_inter) {                                                // U against U in the first tile's lanes, V against V in the second's
            uint32_t cs[16], c_u, c_v;
            v4i w0, w1;
            cost_window(((lane & 31) >> 4) ? s.stile_b : s.stile_a, frag, w0, w1);
            hadamard_pack(H, w0, w1, cs);
            score_tiles(s.ptile, H, cs, lane, frag, c_u, c_v);
            inter_cost = c_u + c_v;
        }
        // one pass scores modes m_a and m_b on both planes
        auto score_pair = [&](int m_a, int m_b, bool have_b, uint32_t &cost_a, uint32_t &cost_b) {
            cost_a = cost_b = 0;
#pragma unroll 1
            for (int plane = 0; plane < 2; ++plane) {
                const unsigned char *raw = plane ? s.raw_b : s.raw_a;
                uint32_t cs[16];
                v4i w0, w1;
                cost_window(plane ? s.stile_b : s.stile_a, frag, w0, w1);
                hadamard_pack(H, w0, w1, cs);
                uint32_t c_a, c_b;
                intra_score_modes(m_a, m_b, have_b, raw, raw + 64, s.ext, s.ptile, H, cs, lane, frag, c_a, c_b);
                cost_a += c_a;
                cost_b += c_b;
            }
        };
        if (DECIDE) {
            // candidates (0, 26, 10, 1[, quadrant 0's mode]): wave w scores positions 2w and 2w + 1; the key carries the position, so the first wins ties
            const int n_cand = q0_intra ? kChromaCandidates : kChromaCandidates - 1;
            uint32_t best_key = 0xFFFFFFFFu;
            if (2 * wave_in_wg < n_cand) {
                const int m_a = wave_in_wg == 0 ? 0 : wave_in_wg == 1 ? 10 : dm_u, m_b = wave_in_wg == 0 ? 26 : 1;
                const bool have_b = 2 * wave_in_wg + 1 < n_cand;
                uint32_t cost_a, cost_b;
                score_pair(m_a, m_b, have_b, cost_a, cost_b);
                best_key = (cost_a << 6) | (uint32_t)(2 * wave_in_wg);
                const uint32_t k_b = have_b ? ((cost_b << 6) | (uint32_t)(2 * wave_in_wg + 1)) : 0xFFFFFFFFu;
                best_key = k_b < best_key ? k_b : best_key;
            }
            if (lane == 0) {
                keys[wave_in_wg] = best_key;
                if (scores_inter) keys[4] = inter_cost;
            }
            __syncthreads();
            if (wave_in_wg != 0) return;
            uint32_t key = keys[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) key = keys[w] < key ? keys[w] : key;
            key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
            const int pos = (int)(key & 63u);
            mode = pos == 0 ? 0 : pos == 1 ? 26 : pos == 2 ? 10 : pos == 3 ? 1 : dm_u;
            intra_cost = key >> 6;
            if (k == 2) inter_cost = (uint32_t)__builtin_amdgcn_readfirstlane((int)keys[4]);
        } else {
            uint32_t unused;
            score_pair(mode, mode, false, intra_cost, unused);
        }
    }
    const bool intra = k == 1 || intra_cost + a.penalty < inter_cost;
    const size_t off = ctu_chroma_tile((size_t)cy, (size_t)cx, c, h, tiles_x) * sizeof(x266_ref_block_t) + ctu_chroma_row_offset(c);
    const v4i a0 = load16<true>(src + off), a1 = load16<true>(src + off + 512);        // tiles 2h and 2h + 1
    const QuantParams qu = region_quant(a.qps, region, a.qp, a.rounding), qv = region_quant(a.qps, region + 1, a.qp, a.rounding);
    if (lane == 0) mixed_region_outputs(a, region, 2, intra ? 1u : 0u, intra ? (unsigned)mode : kInterMode, inter_cost, intra_cost);
    v4i bu, bv;
    if (intra) {
        bu = predict_fragment(mode, s.raw_a, s.ext, s.ptile, lane);
    } else {
        const v4i p0 = load16<true>(prd + off), p1 = load16<true>(prd + off + 512);
        bu = chroma_plane(p0, p1, kSelU);
        bv = chroma_plane(p0, p1, kSelV);
    }
    v4i ou0, ou1, ov0, ov1;
    code_region(chroma_plane(a0, a1, kSelU), bu, kf, ki, c2r, qu, (unsigned)lane, conv, t, dst + 4 * 2048, cnt ? cnt + 4 : nullptr, ou0, ou1);
    __builtin_amdgcn_wave_barrier();                                       // the U levels have left the converter, the U columns the tile
    if (intra) bv = predict_fragment(mode, s.raw_b, s.ext, s.ptile, lane);
    code_region(chroma_plane(a0, a1, kSelV), bv, kf, ki, c2r, qv, (unsigned)lane, conv, t, dst + 5 * 2048, cnt ? cnt + 5 : nullptr, ov0, ov1);
    v4i r0, r1;
    interleave_chroma(recon_luma16(bu, ou0, ou1), recon_luma16(bv, ov0, ov1), r0, r1);
    unsigned char *pr = reinterpret_cast<unsigned char *>(a.recon) + off;
    store16_sc1nt(pr, r0);
    store16_sc1nt(pr + 512, r1);
}

}  // namespace

hipError_t launch_intra32_refs_from_tiles(const x266_ref_block_t *d_frame, int width, int height, int component, x266_intra_ref_t *d_refs,
                                          hipStream_t stream)
{
    const int ctus_x = width / 64, ctus_y = height / 64;
    const size_t n_sets = (size_t)ctus_x * (size_t)ctus_y * (component == 0 ? 4u : 1u);
    if (n_sets == 0) return hipSuccess;
    unsigned wgs;
    if (hipError_t e = wave_grid(n_sets, 4, &wgs)) return e;
    hipLaunchKernelGGL(intra32_refs_from_tiles_kernel, dim3(wgs), dim3(256), 0, stream, d_frame, d_refs, component, ctus_x, ctus_y, n_sets);
    return hipGetLastError();
}

int intra32_frame_steps(int width, int height) { return 4 * (width / 64) + 6 * (height / 64) - 6; }

// one launch per step, on the caller's stream; the CTU rows that have a block at step T are those with 0 <= T - 6 cy < 4 ctus_x
hipError_t launch_intra32_code_frame(const x266_ref_block_t *d_cur, x266_ref_block_t *d_recon, int16_t *d_level, uint32_t *d_nnz, const uint8_t *d_qp,
                                     int qp, int rounding, const uint8_t *d_mode_in, uint8_t *d_mode, int width, int height,
                                     const DctOps *d_fwd_ops, const DctOps *d_inv_acc_ops, hipStream_t stream)
{
    const int ctus_x = width / 64, ctus_y = height / 64;
    const int steps = intra32_frame_steps(width, height);
    for (int step = 0; step < steps; ++step) {
        const int above = step - 4 * ctus_x + 1;                          // cy >= above / 6, rounded up
        const int first = above <= 0 ? 0 : (above + 5) / 6, last = step / 6 < ctus_y - 1 ? step / 6 : ctus_y - 1;
        if (first > last) continue;                                        // a frame one CTU wide has steps without a block
        const dim3 grid((unsigned)(last - first + 1), 2);
        if (d_mode_in)
            hipLaunchKernelGGL(intra_frame_step_kernel<false>, grid, dim3(64), 0, stream, d_cur, d_recon, d_level, d_nnz, d_qp, (unsigned)qp, (unsigned)rounding,
                               d_mode_in, d_mode, ctus_x, ctus_y, step, first, d_fwd_ops, d_inv_acc_ops);
        else
            hipLaunchKernelGGL(intra_frame_step_kernel<true>, grid, dim3(256), 0, stream, d_cur, d_recon, d_level, d_nnz, d_qp, (unsigned)qp, (unsigned)rounding,
                               d_mode_in, d_mode, ctus_x, ctus_y, step, first, d_fwd_ops, d_inv_acc_ops);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// phase 1 (only with kind bytes: without them every region decides), then the steps of the intra frame
hipError_t launch_mixed_code_frame(const x266_mixed_t &p, const DctOps *d_fwd_ops, const DctOps *d_inv_acc_ops, hipStream_t stream)
{
    const int ctus_x = p.width / 64, ctus_y = p.height / 64;
    const size_t n_ctus = (size_t)ctus_x * (size_t)ctus_y;
    const MixedArgs a = {p.d_cur, p.d_pred, p.d_recon, p.d_level, p.d_nnz, p.d_qp, p.d_kind_in, p.d_mode_in, p.d_kind, p.d_mode, p.d_cost,
                         (unsigned)p.qp, (unsigned)p.rounding, (unsigned)p.intra_penalty, ctus_x, ctus_y, d_fwd_ops, d_inv_acc_ops};
    if (p.d_kind_in) {
        unsigned wgs;
        if (hipError_t e = wave_grid(n_ctus * 5, 4, &wgs)) return e;
        hipLaunchKernelGGL(mixed_inter_regions_kernel, dim3(wgs), dim3(256), 0, stream, a, n_ctus);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const int steps = intra32_frame_steps(p.width, p.height);
    for (int step = 0; step < steps; ++step) {
        const int above = step - 4 * ctus_x + 1;
        const int first = above <= 0 ? 0 : (above + 5) / 6, last = step / 6 < ctus_y - 1 ? step / 6 : ctus_y - 1;
        if (first > last) continue;
        const dim3 grid((unsigned)(last - first + 1), 2);
        if (p.d_mode_in) hipLaunchKernelGGL(mixed_frame_step_kernel<false>, grid, dim3(64), 0, stream, a, step, first);
        else hipLaunchKernelGGL(mixed_frame_step_kernel<true>, grid, dim3(256), 0, stream, a, step, first);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace x266
