// x266_device.hpp -- shared device-side types and helpers (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/x266hip.h"
#include "x266_lanes.hpp"             // the cross-lane reductions and scans: every device unit gets them with this header

namespace x266 {

typedef int v4i  __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// 16-byte global accesses; NT = streaming (non-temporal) cache policy.
template <bool NT>
__device__ __forceinline__ v4i load16(const void *p)
{
    const v4i *q = reinterpret_cast<const v4i *>(p);
    if (NT) return __builtin_nontemporal_load(q);
    return *q;
}

template <bool NT>
__device__ __forceinline__ void store16(void *p, const v4i &v)
{
    v4i *q = reinterpret_cast<v4i *>(p);
    if (NT) __builtin_nontemporal_store(v, q);
    else    *q = v;
}

// Streaming store with the cache-policy bits that measured best for write-once output on gfx950
// (profiles/r01_membench_cache_policy.txt: "sc1 nt" copy 6.65 TB/s, "nt" 6.56, default 6.06).  The
// compiler has no spelling for this combination, hence the instruction itself.  The s_nop covers
// the gfx9 hazard "VMEM store of more than 64 bits, then a VALU write of its data VGPRs" (one wait
// state), which the compiler's hazard recognizer cannot see through inline asm -- without it the
// next address computation may overwrite the first 8 bytes of the data still being read.
__device__ __forceinline__ void store16_sc1nt(void *p, const v4i &v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" : : "v"(p), "v"(v));
}

// the same store with agent scope only (no streaming hint): what the WRITE-ONLY intra predictor (long-lived waves) wants -- -1 to -6 % paired on the same
// buffers at 1.0e6 / 2.1e6 / 4.2e6 predictions (profiles/r05_result_stores.txt).  Every kernel with a read stream beside its writes (the transforms, the fused
// intra kernel) and the arithmetic-free copy / write streams themselves are fastest with "sc1 nt"
__device__ __forceinline__ void store16_sc1(void *p, const v4i &v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v));
}

// ---- hand-counted waits ---------------------------------------------------------------------------------------------------
// The LDS-DMA kernels (dct32_fwdinv_kernel, satd8x8_dma_kernel, satd8x8_from_tiles_dma_kernel) issue their loads and streaming stores as
// inline asm, invisible to the compiler's vmcnt bookkeeping, and wait by COUNT: a wave's vector memory operations retire in issue
// order, so "fetch f has landed" = at most {the operations issued after f} outstanding.  Every such count is written as a sum of
// the per-call instruction counts below (kDmaPer*, kStoresPer*), which the issuing helpers static_assert against what they emit.
// The check that the sums are right is by execution: `make -C x266_amd/csrc waits0` builds libx266hip_waits0.so with X266_WAIT_ALL,
// where every counted wait waits for EVERYTHING, and tests/test_gpu_waits.py compares the two libraries byte for byte on ragged,
// steady-state and single-block runs -- a count that is too high reads an LDS slot before its DMA landed and shows there.
__device__ __forceinline__ void wait_vmcnt(unsigned n)
{
#ifdef X266_WAIT_ALL
    (void)n;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    switch (n) {
#define X266_WAIT(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    X266_WAIT(1) X266_WAIT(2) X266_WAIT(3) X266_WAIT(4) X266_WAIT(5) X266_WAIT(6) X266_WAIT(7) X266_WAIT(8) X266_WAIT(9) X266_WAIT(10)
    X266_WAIT(11) X266_WAIT(12) X266_WAIT(13) X266_WAIT(14) X266_WAIT(15) X266_WAIT(16) X266_WAIT(17) X266_WAIT(18) X266_WAIT(19) X266_WAIT(20)
    X266_WAIT(21) X266_WAIT(22) X266_WAIT(23) X266_WAIT(24) X266_WAIT(25) X266_WAIT(26) X266_WAIT(27) X266_WAIT(28) X266_WAIT(29) X266_WAIT(30)
    X266_WAIT(31) X266_WAIT(32) X266_WAIT(33) X266_WAIT(34) X266_WAIT(35) X266_WAIT(36) X266_WAIT(37) X266_WAIT(38) X266_WAIT(39) X266_WAIT(40)
#undef X266_WAIT
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // 0, and anything beyond the counter's range
    }
#endif
}
constexpr unsigned kWaitVmcntMax = 40;

// Byte i of a read-only table of any alignment, for a wave-uniform i, as a wave-uniform value: the aligned dword that holds it is
// read through a constant-address-space pointer, which the compiler turns into s_load_dword (a pointer made from an integer is
// otherwise a generic one and costs a flat_load and a vector-memory round trip), and readfirstlane pins the result to an SGPR so
// that whatever is derived from it runs on the scalar ALU.  Class and qp bytes are read this way.
__device__ __forceinline__ unsigned uniform_byte(const uint8_t *table, size_t i)
{
    typedef const __attribute__((address_space(4))) uint32_t *const_dword_ptr;
    const uintptr_t a = reinterpret_cast<uintptr_t>(table) + i;
    const uint32_t w = *(const_dword_ptr)(a & ~(uintptr_t)3);
    return ((uint32_t)__builtin_amdgcn_readfirstlane((int)w) >> (8 * (unsigned)(a & 3))) & 255u;
}

// Result streams -- a few bytes written per hundred read (SATD / SAD costs): agent-scope "sc1" stores without the streaming hint.  Measured on
// the SATD batch, paired over eight allocation sets (profiles/r05_result_stores.txt): plain or sc0 0.360 ms, nt 0.334-0.360, sc1 nt 0.329-0.339,
// sc1 or sc0 sc1 0.325-0.330 -- and the kernel no longer follows where its small output buffer landed.
__device__ __forceinline__ void store_result16(void *p, const v4i &v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_result4(uint32_t *p, uint32_t v)    // a relaxed agent-scope store IS "global_store_dword ... sc1", and the compiler still counts it
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// SM: 0 plain, 1 nontemporal, 2 "sc1 nt"
template <int SM>
__device__ __forceinline__ void store16m(void *p, const v4i &v)
{
    if (SM == 2) store16_sc1nt(p, v);
    else         store16<SM == 1>(p, v);
}

struct LaunchCfg {
    int cu_count;             // compute units of the device
    int adaptive;             // shrink units_per_wave on small batches so the grid still fills the chip
    int units_per_wave;       // streaming launch: consecutive units (DCT blocks / 32-block SATD groups / tiles) per wave; SATD batch: 0 = the kernel's own default
    int wg_threads;           // workgroup size, multiple of 64; SATD batch: 0 = the kernel's own default
    int lds_bytes_per_wave;   // LDS charged per wave (what the kernel uses + padding): 160 KiB / this = cap on resident waves per CU; SATD batch: 0 = default
    int shape;                // SATD batch: 0 kernel by batch size, 1 staged kernel, 3 LDS-DMA kernel; fused forward + inverse: input slots per wave (0 = 2, or 3)
};

// SATD batch: from this many blocks on the LDS-DMA kernel runs (satd_kernels.hip, launch_satd8x8)
constexpr size_t kSatdDmaMinBlocks = (size_t)3 << 20;

struct DctOps;
struct TileTab;

// Units (blocks, groups, tiles) one wave loops over: the configured count, reduced on small batches
// until the launch has at least two full rounds of resident waves (about 40 per CU).
inline unsigned units_per_wave_for(const LaunchCfg &cfg, size_t n_units)
{
    unsigned u = cfg.units_per_wave < 1 ? 1u : (unsigned)cfg.units_per_wave;
    if (cfg.adaptive) {
        const size_t fill = (size_t)cfg.cu_count * 40u;
        const size_t cap = n_units / fill;
        if (cap < u) u = cap < 1 ? 1u : (unsigned)cap;
    }
    return u;
}

// Workgroups of a one-dimensional grid of n_waves waves, waves_per_wg to a workgroup; a grid dimension holds 2^31 - 1 at most
inline hipError_t wave_grid(size_t n_waves, size_t waves_per_wg, unsigned *wgs)
{
    const size_t n = (n_waves + waves_per_wg - 1) / waves_per_wg;
    if (n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    *wgs = (unsigned)n;
    return hipSuccess;
}

hipError_t launch_intra32_predict(const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index,
                                  uint8_t *d_pred, size_t n, int rounds, hipStream_t stream);
hipError_t launch_intra32_residual_dct32(const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index, const uint8_t *d_src,
                                         int16_t *d_coef, size_t n, const DctOps *d_fwd_ops, hipStream_t stream);
hipError_t launch_intra32_costs(const x266_intra_ref_t *d_refs, const uint8_t *d_src, uint32_t *d_costs, uint8_t *d_best_mode,
                                size_t n, hipStream_t stream);
// the sets of a tiled frame's own samples (component 0: four per CTU; 1 / 2: one), and the closed-loop intra coding of a frame: one launch per step
hipError_t launch_intra32_refs_from_tiles(const x266_ref_block_t *d_frame, int width, int height, int component, x266_intra_ref_t *d_refs,
                                          hipStream_t stream);
int intra32_frame_steps(int width, int height);
hipError_t launch_intra32_code_frame(const x266_ref_block_t *d_cur, x266_ref_block_t *d_recon, int16_t *d_level, uint32_t *d_nnz, const uint8_t *d_qp,
                                     int qp, int rounding, const uint8_t *d_mode_in, uint8_t *d_mode, int width, int height,
                                     const DctOps *d_fwd_ops, const DctOps *d_inv_acc_ops, hipStream_t stream);
// mixed inter / intra coding of a frame: one launch for the regions given as inter, then the steps of the intra frame
hipError_t launch_mixed_code_frame(const x266_mixed_t &p, const DctOps *d_fwd_ops, const DctOps *d_inv_acc_ops, hipStream_t stream);
hipError_t launch_satd8x8_butterfly(const int16_t *d_diff, uint32_t *d_out, size_t n_blocks, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_transform_tiles(bool inverse, const int16_t *d_in, int16_t *d_out, size_t n_tiles, const uint32_t *d_tile_offsets,
                                  const uint8_t *d_tile_class, const TileTab *d_tab, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_transform_ctu_tiles(bool inverse, const x266_ref_block_t *d_cur, const int16_t *d_coef_in, const x266_ref_block_t *d_pred,
                                      const uint8_t *d_class, int16_t *d_coef_out, x266_ref_block_t *d_recon, int width, int height,
                                      const TileTab *d_tab, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32_butterfly(const int16_t *d_in, int16_t *d_out, size_t n_blocks, hipStream_t stream);
hipError_t launch_dct32_pass(const int16_t *d_in, int16_t *d_out, size_t n_blocks, int shift, const DctOps *d_fwd_ops, hipStream_t stream);
hipError_t launch_dct32_fwdinv(const int16_t *d_in, int16_t *d_coef, int16_t *d_recon, size_t n_blocks,
                               const DctOps *d_fwd_ops, const DctOps *d_inv_acc_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32(bool inverse, const int16_t *d_in, int16_t *d_out, size_t n_blocks,
                        const DctOps *d_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_transform_small(int log2n, const int16_t *d_in, int16_t *d_out, size_t n_blocks, const DctOps *d_ops,
                                  const uint32_t *d_offsets, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32_from_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_out,
                                   int width, int height, const DctOps *d_fwd_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_transform_small_inv(int log2n, const int16_t *d_in, int16_t *d_out, size_t n_blocks, const DctOps *d_ops,
                                      const uint32_t *d_offsets, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_satd8x8_from_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, uint32_t *d_out,
                                     int width, int height, int shape, hipStream_t stream);
hipError_t launch_frame_lanes(const int16_t *d_dct_in, int16_t *d_dct_out, size_t n_dct, const DctOps *d_fwd_ops,
                              const int16_t *d_diff, uint32_t *d_satd_out, size_t n_satd, const LaunchCfg &satd_cfg, hipStream_t stream);
hipError_t launch_satd8x8(const int16_t *d_diff, uint32_t *d_out, size_t n_blocks,
                          const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_satd_search(const uint8_t *d_cur, long long cur_stride, const uint8_t *d_ref, long long ref_stride,
                               int width, int height, int range, x266_me_result_t *d_best, uint32_t *d_costs,
                               int tile_rows, uint32_t *d_coef_scratch, int cu_count, bool tiled, hipStream_t stream);
hipError_t launch_sad_search(const uint8_t *d_cur, long long cur_stride, const uint8_t *d_ref, long long ref_stride,
                              int width, int height, int range, x266_me_result_t *d_best, uint32_t *d_costs,
                              int tile_rows, bool tiled, hipStream_t stream);
hipError_t launch_sad(int edge, const uint8_t *d_a, const uint8_t *d_b, uint32_t *d_out, size_t n_blocks, int waves_per_wg, int lds_per_wg, hipStream_t stream);
hipError_t launch_tile_convert(bool pack, x266_ref_block_t *d_tiles, uint8_t *d_y, uint8_t *d_u, uint8_t *d_v,
                               long long strd_y, long long strd_c, int width, int height, hipStream_t stream);
hipError_t launch_residual_luma(int block_edge, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_res,
                                int width, int height, hipStream_t stream);
hipError_t launch_residual_chroma(int block_edge, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_res_u, int16_t *d_res_v,
                                  size_t block_pitch, int width, int height, hipStream_t stream);
hipError_t launch_dct32_chroma_from_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_out_u, int16_t *d_out_v,
                                          size_t block_pitch, int width, int height, const DctOps *d_fwd_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32_ctu_from_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int16_t *d_out,
                                       int width, int height, const DctOps *d_fwd_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_satd8x8_chroma_from_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, uint32_t *d_out_u, uint32_t *d_out_v,
                                            size_t pitch, int width, int height, hipStream_t stream);
hipError_t launch_recon_luma(int block_edge, const x266_ref_block_t *d_pred, const int16_t *d_res, x266_ref_block_t *d_recon,
                             int width, int height, hipStream_t stream);
hipError_t launch_recon_chroma(int block_edge, const x266_ref_block_t *d_pred, const int16_t *d_res_u, const int16_t *d_res_v, size_t block_pitch,
                               x266_ref_block_t *d_recon, int width, int height, hipStream_t stream);
hipError_t launch_dct32_inv_to_tiles(const int16_t *d_coef, const x266_ref_block_t *d_pred, x266_ref_block_t *d_recon, int width, int height,
                                     const DctOps *d_inv_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32_inv_ctu_to_tiles(const int16_t *d_coef, const x266_ref_block_t *d_pred, x266_ref_block_t *d_recon, int width, int height,
                                         const DctOps *d_inv_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_dct32_code_ctu_tiles(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, x266_ref_block_t *d_recon, int16_t *d_level,
                                       uint32_t *d_nnz, const uint8_t *d_qp, int qp, int rounding, int width, int height, const DctOps *d_fwd_ops,
                                       const DctOps *d_inv_acc_ops, const LaunchCfg &cfg, hipStream_t stream);
hipError_t launch_quant_regions(bool inverse, const int16_t *d_in, int16_t *d_out, size_t n_regions, const uint8_t *d_class,
                                const uint8_t *d_qp, int qp, int rounding, uint32_t *d_nnz, hipStream_t stream);
hipError_t launch_motion_comp_luma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                                   int width, int height, hipStream_t stream);
hipError_t launch_motion_comp_chroma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                                     int width, int height, hipStream_t stream);
hipError_t launch_motion_comp(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred,
                              int width, int height, hipStream_t stream);
hipError_t launch_mc_qpel_luma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                               hipStream_t stream);
hipError_t launch_mc_qpel_chroma(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                                 hipStream_t stream);
hipError_t launch_mc_qpel(const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, x266_ref_block_t *d_pred, int width, int height,
                          hipStream_t stream);
hipError_t launch_satd_refine_qpel(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref, int width, int height,
                                   const x266_me_result_t *d_int, x266_me_result_t *d_best, uint32_t *d_costs, hipStream_t stream);
// bi-directional: planes 1 = m_Y, 2 = m_C, 3 = both; wp is never NULL here (the entry points fill in the default weights)
hipError_t launch_mc_bi_qpel(int planes, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, const x266_me_result_t *d_mv0,
                             const x266_me_result_t *d_mv1, const uint8_t *d_dir, const x266_wp_t &wp, x266_ref_block_t *d_pred, int width, int height,
                             hipStream_t stream);
hipError_t launch_satd_bi_costs(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, int width, int height,
                                const x266_me_result_t *d_mv0, const x266_me_result_t *d_mv1, const x266_wp_t &wp, int bi_penalty, uint32_t *d_costs,
                                uint8_t *d_dir, hipStream_t stream);
hipError_t launch_satd_refine_bi_qpel(const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref_fix, const x266_me_result_t *d_mv_fix,
                                      const x266_ref_block_t *d_ref, const x266_me_result_t *d_int, int list, const x266_wp_t &wp, int width, int height,
                                      x266_me_result_t *d_best, uint32_t *d_costs, hipStream_t stream);
// planes: 1 = m_Y, 2 = m_C, 3 = both in one launch
hipError_t launch_deblock(int planes, const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const x266_deblock_t &p,
                          hipStream_t stream);
// d_param NULL: statistics only; otherwise statistics and decision in one launch, and d_stats may be NULL
hipError_t launch_sao_stats(const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, int lambda_q4, int32_t *d_stats,
                            x266_sao_t *d_param, hipStream_t stream);
hipError_t launch_sao_decide(const int32_t *d_stats, size_t n_ctu, int lambda_q4, x266_sao_t *d_param, hipStream_t stream);
hipError_t launch_sao_apply(const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const x266_sao_t *d_param, hipStream_t stream);
// adaptive loop filter (alf_kernels.hip); d_class NULL in the statistics and in apply: classified inside
hipError_t launch_alf_classify(const x266_ref_block_t *d_dec, int width, int height, uint8_t *d_class, hipStream_t stream);
hipError_t launch_alf_stats(const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, const uint8_t *d_class, int32_t *d_stats,
                            hipStream_t stream);
hipError_t launch_alf_sum_stats(const int32_t *d_stats, size_t n_ctu, const uint8_t *d_mask, int64_t *d_total, hipStream_t stream);
hipError_t launch_alf_decide(const int32_t *d_stats, size_t n_ctu, const x266_alf_luma_t *d_luma, int n_luma, const x266_alf_chroma_t *d_chroma, int n_chroma,
                             int lambda_q4, uint8_t *d_ctrl, hipStream_t stream);
hipError_t launch_alf_apply(const x266_ref_block_t *d_in, x266_ref_block_t *d_out, int width, int height, const uint8_t *d_class, const x266_alf_luma_t *d_luma,
                            int n_luma, const x266_alf_chroma_t *d_chroma, int n_chroma, const uint8_t *d_ctrl, hipStream_t stream);
// the compact level stream (levels_kernels.hip): pack = count, scan, write on one stream; the scan's step is levels_scan_chunk() regions
hipError_t launch_levels_pack(const x266_levels_t &p, hipStream_t stream);
hipError_t launch_levels_unpack(const x266_levels_t &p, hipStream_t stream);
unsigned levels_scan_chunk();
// RDOQ and the level rate estimate (rdoq_kernels.hip): one launch each
hipError_t launch_rdo_quant_regions(const x266_rdoq_t &p, hipStream_t stream);
hipError_t launch_levels_bits(const x266_rdoq_t &p, hipStream_t stream);
// the transform decision (rdoq_kernels.hip): one launch, one region per wave; d_tab is the forward TileTab
hipError_t launch_transform_decide(const x266_tdecide_t &p, const TileTab *d_tab, hipStream_t stream);
// source analysis (aq_kernels.hip): stats = the tile records, then the totals' one workgroup of aq_totals_chunk() records per step
hipError_t launch_aq_stats(const x266_aq_t &p, hipStream_t stream);
hipError_t launch_aq_decide(const x266_aq_t &p, hipStream_t stream);
int aq_totals_chunk();
// frame quality (quality_kernels.hip): the CTU records, then (d_total given) the totals' one workgroup of quality_totals_chunk() records per step
hipError_t launch_quality_stats(const x266_quality_t &p, hipStream_t stream);
int quality_totals_chunk();
// the lookahead (lookahead_kernels.hip): frame cost = the block records, then the totals' one workgroup of la_totals_chunk() blocks per step
hipError_t launch_la_downscale(const x266_la_t &p, hipStream_t stream);
hipError_t launch_la_intra_costs(const x266_la_t &p, hipStream_t stream);
hipError_t launch_la_frame_cost(const x266_la_t &p, hipStream_t stream);
hipError_t launch_la_propagate(const x266_la_t &p, hipStream_t stream);
hipError_t launch_la_tree_qp(const x266_la_t &p, hipStream_t stream);
int la_totals_chunk();
// the seeded search (seeded_search_kernels.hip): one launch, one wave per seed cell, no scratch
hipError_t launch_seeded_search(const x266_seed_t &p, hipStream_t stream);
// the inter partition decision (partition_kernels.hip): one launch, one workgroup per CTU, no scratch
hipError_t launch_partition_decide(const x266_part_t &p, hipStream_t stream);
// the compact motion stream (motion_kernels.hip): pack = count, the level stream's offset scan, write on one stream; unpack is one launch
hipError_t launch_motion_pack(const x266_motion_t &p, hipStream_t stream);
hipError_t launch_motion_unpack(const x266_motion_t &p, hipStream_t stream);
// the vectors from the differences: one launch per wavefront step cx + 2 cy, one wave per CTU of the step, stream order alone
hipError_t launch_motion_reconstruct(const x266_motion_t &p, hipStream_t stream);
// the entropy coder of the level stream (entropy_kernels.hip): encode = count, the level stream's offset scan, write on one stream; decode is one launch
hipError_t launch_entropy_encode(const x266_entropy_t &p, hipStream_t stream);
hipError_t launch_entropy_decode(const x266_entropy_t &p, hipStream_t stream);
// the entropy coder of the motion stream (entropy_kernels.hip): the same three launches on x266_entropy_motion_ctu_t; decode is one launch
hipError_t launch_entropy_motion_encode(const x266_entropy_motion_t &p, hipStream_t stream);
hipError_t launch_entropy_motion_decode(const x266_entropy_motion_t &p, hipStream_t stream);
// the entropy coder of the side information (entropy_side_kernels.hip): the same three launches on x266_entropy_side_ctu_t, one lane per CTU; decode is one launch
hipError_t launch_entropy_side_encode(const x266_entropy_side_t &p, hipStream_t stream);
hipError_t launch_entropy_side_decode(const x266_entropy_side_t &p, hipStream_t stream);
// the per-context bin statistics (entropy_stats_kernels.hip): the rows, then one workgroup adding them in ascending order
hipError_t launch_entropy_stats_levels(const x266_entropy_stats_t &p, hipStream_t stream);
hipError_t launch_entropy_stats_side(const x266_entropy_side_stats_t &p, hipStream_t stream);
hipError_t launch_mem_ceiling(int kind, const void *d_src, void *d_dst, size_t bytes, hipStream_t stream);
hipError_t launch_fill_residual(int16_t *d_dst, size_t n_samples, uint64_t seed,
                                uint64_t first_index, const LaunchCfg &cfg, hipStream_t stream);

}  // namespace x266
