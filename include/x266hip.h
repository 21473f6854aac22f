/*
 * x266hip.h -- C ABI of libx266hip.so: the MI355X (gfx950) implementation of
 * x266's block-transform / motion-cost hot path.
 *
 * Plain C, plain pointers and sizes; no HIP, torch or C++ types cross this
 * boundary (a stream is passed as an opaque `void *` that holds a hipStream_t).
 * Reference paths below are relative to the upstream x266 tree.
 *
 * Four groups of entry points:
 *
 *  1. The six BDPI symbols the Bluespec testbenches import
 *     (src/mkDct32.bsv:409-411, src/mkSatd.bsv:204-206) and that upstream
 *     defines in src_tb/dct32.c:178-246 and src_tb/satd.c:124-152.  Signatures,
 *     packing, call order and statefulness are identical, so this library can
 *     replace src_tb/{dct32,satd}.c on the bsc link line that names every src_tb C file
 *     link line (build/Makefile:65-67); the golden values the DUT is compared
 *     with are then computed by the GPU kernels.
 *
 *  2. Batch entry points (no upstream counterpart -- upstream is one block at
 *     a time).  Conventions follow src/x266.cpp: `x` prefix, context first,
 *     caller-allocated buffers, int 0 / negative return (x266.cpp:494-513).
 *     Block layout is the reference's: row-major int16, blocks contiguous
 *     (32x32 = 2048 B per DCT block, 8x8 = 128 B per SATD block).
 *
 *  3. Small host utilities (word packing, device memory, streams, events,
 *     graphs) so that a pure-C host can drive the device-pointer API without
 *     HIP headers.
 *
 *  4. One node, several GPUs (BASELINE configs[4]): shards of a batch, a
 *     pipelined frame stream and a striped motion search over RCCL send/recv
 *     groups.  A node and its streams are driven by one host thread at a time.
 *
 * The library NEVER falls back to a CPU implementation: without a usable
 * gfx950 device every compute entry point fails (negative return; the BDPI
 * shims print to stderr and abort()).
 */
#ifndef X266HIP_H
#define X266HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* return codes (x266.cpp style: 0 ok, negative failure)                     */
/* ------------------------------------------------------------------------ */
#define X266HIP_OK        0
/* X266HIP_EINVAL from a device call: nothing was launched, and xHipLastError says "<entry point>: <the rule broken>"; the rules
 * of every device call (NULL, alignment, spans, overlap, sizes, scalar ranges) are those of x266_amd/csrc/x266_args.hpp. */
#define X266HIP_EINVAL   (-1)   /* bad argument (NULL pointer with n > 0, ...)  */
#define X266HIP_EDEVICE  (-2)   /* no gfx950 device / HIP runtime error         */
#define X266HIP_ENOMEM   (-3)   /* device or host allocation failed             */

typedef struct x266hip_ctx x266hip_ctx;     /* opaque, one per (thread, device) */

/* ------------------------------------------------------------------------ */
/* context (cf. xCodecInit / xCodecFree, src/x266.cpp:494-524)               */
/* ------------------------------------------------------------------------ */
/* Creates a context on HIP device `device_id`, uploads the MFMA operand images
 * of the coefficient matrix (g_t32, src_tb/dct32.c:30-64).  Fails with
 * X266HIP_EDEVICE when the device is not a gfx950 part. */
int  xHipCodecInit(x266hip_ctx **ctx, int device_id);
/* Number of HIP devices visible to the process (0 when there is none or the runtime fails). */
int  xHipDeviceCount(void);
void xHipCodecFree(x266hip_ctx *ctx);
/* Last error text of this context (never NULL; "" when none). */
const char *xHipLastError(const x266hip_ctx *ctx);
/* Device facts for reports: name, CU count, max engine clock (MHz), HBM bytes. */
int  xHipDeviceInfo(const x266hip_ctx *ctx, char *name, size_t name_cap,
                    int *cu_count, int *clock_mhz, size_t *hbm_bytes);
/* Launch options, for A/B measurement (defaults are the measured optimum; results never depend on them; unknown keys and
 * out-of-range values return X266HIP_EINVAL).  The complete list (the kOptions table of x266_amd/csrc/x266hip_abi.hip):
 *   "dct32_variant"          0 matrix-core kernel, 2 the reference's even/odd butterfly on the vector ALU
 *   "satd_variant"           0 by batch size (staged kernel below 3 Mi blocks, LDS-DMA kernel from there on), 1 staged kernel,
 *                            2 radix-2 butterflies on the vector ALU, 3 LDS-DMA kernel
 *                            (2 = the one comparison variant per kernel family north_star asks for)
 *   "dct32_blocks_per_wave", "dct32_inv_blocks_per_wave", "dct32_fwdinv_blocks_per_wave" (1 / 2 / 0 = automatic: 2, or 8 when d_coef is NULL)
 *                            consecutive blocks (tiles, for the transform set's inverses) one wave loops over
 *   "dct32_wg_threads"       workgroup size of the calls listed below (64, 128, 192, 256; default 0 = the measured
 *                            best: 64, and 256 for the fused forward + inverse kernel)
 *   "satd_groups_per_wave", "satd_wg_threads", "satd_lds_bytes_per_wave"
 *                            SATD batch: 32-block groups per wave, workgroup size, LDS charged per wave (= cap on resident
 *                            waves per CU); 0 (default) = the chosen kernel's own: 2 / 128 / 6144 staged, 4 / 256 / 16384 LDS-DMA.
 *                            "satd_lds_bytes_per_wave" takes 0 .. 16384 in multiples of 16 (whole 16-byte rows; 16 KiB x the four waves of
 *                            the largest workgroup = the 64 KiB a launch may ask for; values below the kernel's own need are raised to it)
 *   "tile_tiles_per_wave"    xTransformTilesDev: consecutive tiles per wave (0 = 2)
 *   "adaptive_per_wave"      shrink the per-wave run on small batches (default 1): a per-wave count is cut to units / (CU count x 40), at
 *                            least 1, so below CU count x 40 x 2 units (20 480 on 256 CUs) a per-wave option has NO effect unless this is 0
 *   "me_tile_rows"           motion-search tile height in block rows (0, the default: chosen from the frame size and the CU count);
 *                            applies to xSatd8x8SearchDev / xSad8x8SearchDev and their tiled forms ...SearchFromTilesDev alike
 *   "autotune"               0 (default) / 1: boxes differ in which launch shape a few kernels run fastest in (by up to 5 %).  With 1, the FIRST
 *                            large call of a family -- xDct32FwdInvBatchDev with and without d_coef (>= 2^18 blocks), xSatd8x8BatchDev
 *                            (>= 2^23 blocks), xSadBatchDev edge >= 8 (>= 128 MiB per input) -- times the family's candidate shapes on the
 *                            caller's own buffers and stream (that one call is synchronous: 4 launches per candidate shape plus the final
 *                            one, 33 for the 8 shapes of the first family; every launch writes the same bytes) and the context keeps the
 *                            fastest (the default unless beaten by > 2 %); xHipAutotuneReport shows what was measured.  Skipped under
 *                            stream capture, for overlapping buffers and when the family's own knobs are set ("satd_variant" included).
 *                            2 + k (k = 0 .. 8) is a test hook: every call of these families, at any batch size > 0, launches candidate
 *                            k of its table -- no timing, so also under capture; the same calls as above keep the default shape -- and
 *                            a family with k or fewer candidates (8 / 5 / 6 / 5) returns X266HIP_EINVAL and launches nothing.
 *                            Setting the option to any value forgets what the context has tuned or counted so far.
 * The calls that take each option (what one wave takes is a 32x32 block, a tile, a 32-block SATD group; tests/_option_cases.py holds
 * this list as a table and tests/test_gpu_options.py runs it; the "autotune" families are named above):
 *   "dct32_variant":                xDct32FwdBatchDev, xDct32FwdBatch, xTransformFwdBatchDev (contiguous 32x32 batches)
 *   "dct32_blocks_per_wave":        xDct32FwdBatchDev, xDct32FwdBatch, xTransformFwdBatchDev (contiguous 32x32 batches; else one tile per wave)
 *   "dct32_inv_blocks_per_wave":    xDct32InvBatchDev, xDct32InvBatch, xTransformInvBatchDev, xDct32InvToTilesDev
 *   "dct32_fwdinv_blocks_per_wave": xDct32FwdInvBatchDev
 *   "dct32_wg_threads":             xDct32FwdBatchDev, xDct32FwdBatch, xDct32InvBatchDev, xDct32InvBatch, xDct32FwdInvBatchDev,
 *                                   xTransformFwdBatchDev, xTransformInvBatchDev, xTransformTilesDev, xDct32FwdFromTilesDev,
 *                                   xDct32FwdChromaFromTilesDev, xDct32FwdCtuFromTilesDev, xDct32InvToTilesDev, xDct32InvCtuToTilesDev,
 *                                   xDct32CodeCtuTilesGpu, xTransformCtuFromTilesDev, xTransformCtuToTilesDev
 *   "satd_variant":                 xSatd8x8BatchDev, xSatd8x8Batch, xSatd8x8FromTilesDev (0 / 1 / 3; 2 runs as 0)
 *   "satd_groups_per_wave":         xSatd8x8BatchDev, xSatd8x8Batch, xDct32SatdFrameDev (the staged body in two-wave workgroups: 0 = 2)
 *   "satd_wg_threads":              xSatd8x8BatchDev, xSatd8x8Batch
 *   "satd_lds_bytes_per_wave":      xSatd8x8BatchDev, xSatd8x8Batch
 *   "tile_tiles_per_wave":          xTransformTilesDev
 *   "adaptive_per_wave":            every call above that takes a per-wave option
 *   "me_tile_rows":                 xSatd8x8SearchDev, xSatd8x8SearchFromTilesDev (0, or snapped to 2 / 4 / 8: 1 and 3 run 2, 5 .. 7 run 4);
 *                                   xSad8x8SearchDev, xSad8x8SearchFromTilesDev (two block rows whatever the value)
 * Rounds 1-3 had sixteen more (cache-policy bits, LDS staging on / off, padding, per-kernel LDS charges, ...): the forms they
 * selected lost their A/Bs (profiles/r01_*.txt) and are gone. */
int  xHipSetOption(x266hip_ctx *ctx, const char *key, int value);
int  xHipGetOption(const x266hip_ctx *ctx, const char *key, int *value);
/* "autotune": one text line per tuned family -- "<family> choice <index> ms <per-candidate milliseconds, -1 = not launchable>" --
 * candidate 0 being the default shape (x266_amd/csrc/x266hip_abi.hip, k*Cands); under "autotune" = 2 + k one line per family
 * that has launched since the option was set -- "<family> forced <k> launches <number of launches that took candidate k>".
 * Families: dct32_fwd_inv, dct32_recon_only, satd8x8, sad8, sad16, sad32, sad64.  A `cap` that does not hold the whole text and
 * its terminator returns X266HIP_EINVAL (buf[0] = 0): never a cut line. */
int  xHipAutotuneReport(const x266hip_ctx *ctx, char *buf, size_t cap);

/* ------------------------------------------------------------------------ */
/* batch API, device pointers (inputs already resident in HBM)               */
/* `stream` holds a hipStream_t (NULL = the default stream).  Asynchronous:  */
/* returns after enqueueing; use xHipStreamSync or the caller's own stream   */
/* API to wait.  Inputs and outputs must not overlap unless a call says so.   */
/* ------------------------------------------------------------------------ */
/* Alignment: every device entry point below -- a call that takes the context first, the stream last and device buffers in
 * between -- is preceded by an "Alignment in bytes" line that names each of its device pointers (for the deblocking calls:
 * d_in, d_out and the pointer fields of x266_deblock_t) with the alignment the call's argument check enforces (1 = none;
 * tests/test_arg_rules.py holds every line against the rules); a pointer aligned to less returns
 * X266HIP_EINVAL and launches nothing, and nothing MORE than that alignment is needed -- sample, coefficient and tile buffers
 * 16, x266_me_result_t records and the chroma planes of the two conversion calls 8, uint32_t outputs and index / offset
 * tables 4 (the SATD output of xDct32SatdFrameDev: 16), mode and class bytes and the pixel planes of the planar searches none
 * (the current plane of xSad8x8SearchDev: 4).
 * tests/test_gpu_placement.py runs every ...Dev call at exactly these alignments and checks their lines against its table.
 * A call reads nothing whose value can reach its result outside the documented extent of its inputs, and writes nothing
 * outside the documented extent of its outputs. */
/* 2-D forward 32x32 DCT-II, shifts 4 then 11, truncating int16 stores:
 * bit-exact with partialButterfly32 x2 as called by dct32_genNew
 * (src_tb/dct32.c:66-170,180-198).  out[v*32+u], v = vertical frequency. */
/* Alignment in bytes: d_in 16, d_out 16. */
int xDct32FwdBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out,
                      size_t n_blocks, void *stream);
/* 2-D inverse (no upstream counterpart; HEVC/VVC inverse for 8-bit video:
 * column pass shift 7, row pass shift 12, int16 clipping after each pass). */
/* Alignment in bytes: d_in 16, d_out 16. */
int xDct32InvBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out,
                      size_t n_blocks, void *stream);
/* The two lanes of a frame in ONE launch: xDct32FwdBatchDev of one batch and xSatd8x8BatchDev of another, bit-identical
 * to the two calls (BASELINE configs[4]: a 7680x4320 frame is 32 400 DCT32 blocks + 518 400 SATD blocks, ~15 us of kernel
 * each -- submissions, not arithmetic, pace a frame stream on one GPU).  Either count may be 0.  All four buffers are checked
 * for 16 bytes here, d_satd_out included (xSatd8x8BatchDev alone takes it at 4). */
/* Alignment in bytes: d_dct_in 16, d_dct_out 16, d_diff 16, d_satd_out 16. */
int xDct32SatdFrameDev(x266hip_ctx *ctx, const int16_t *d_dct_in, int16_t *d_dct_out, size_t n_dct_blocks,
                       const int16_t *d_diff, uint32_t *d_satd_out, size_t n_satd_blocks, void *stream);
/* The 1-D pass by itself: partialButterfly32(src, dst, shift, line = 32) (src_tb/dct32.c:66-170; the RTL's first stage,
 * src/mkDct32.bsv:213-284) on every 32x32 block of the batch, i.e. dst[k*32 + j] = (int16)((sum_n g_t32[k][n] *
 * src[j*32 + n] + (1 << (shift-1))) >> shift) -- note the TRANSPOSED store.  xDct32PassDev(shift 4) followed by
 * xDct32PassDev(shift 11) is xDct32FwdBatchDev; on its own it lets a testbench compare the intermediate of a DUT.
 * Exact for every int16 input at shifts 1..15.  (A checking entry point: one block per wave, not a tuned kernel.) */
/* Alignment in bytes: d_in 16, d_out 16. */
int xDct32PassDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out, size_t n_blocks, int shift, void *stream);
/* Forward and inverse in one pass over the batch: d_coef = forward(d_in) (may be NULL when only
 * the reconstruction is wanted), d_recon = inverse(forward(d_in)) -- the transform half of an
 * encoder's reconstruction loop; SURVEY 8(d) "fused fwd+inv", 6144 bytes per block instead of
 * 8192.  Bit-identical to xDct32FwdBatchDev followed by xDct32InvBatchDev. */
/* Alignment in bytes: d_in 16, d_coef 16, d_recon 16. */
int xDct32FwdInvBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_coef, int16_t *d_recon,
                         size_t n_blocks, void *stream);
/* 8x8 Hadamard SATD of n residual blocks: bit-exact with satd8x8
 * (src_tb/satd.c:31-118), including its int16 wraparound.  d_out[n] uint32, 4-byte aligned (d_diff 16). */
/* Alignment in bytes: d_diff 16, d_out 4. */
int xSatd8x8BatchDev(x266hip_ctx *ctx, const int16_t *d_diff, uint32_t *d_out,
                     size_t n_blocks, void *stream);
/* The mixed transform set of BASELINE configs[3]: forward 2-D transforms of square N x N
 * int16 blocks (row-major, N*N samples each) built from two 1-D transform SLOTS: slot 0 with
 * N in {4, 8, 16, 32}, by default the DCT-II (sub-matrices of g_t32; N = 32 is pinned by the reference),
 * and slot 1 with N in {4, 8, 16}, by default the closed-form DST-VII
 * round(64 sqrt(N) sqrt(4/(2N+1)) sin(pi (2k+1)(n+1)/(2N+1))) -- for N = 4 the table of H.266, for N = 8 / 16
 * NOT claimed to be the standard's integers (those could not be checked offline; a host that holds the
 * normative tables, or wants DCT-VIII, installs them with xTransformSetMatrix below).
 * Two passes with partialButterfly32's structure
 * (src_tb/dct32.c:66-170): rows then columns, shifts log2N-1 and log2N+6, rounding
 * half up, truncating int16 stores; the DCT-II matrices are the sub-matrices of g_t32
 * that src/mkDct32.bsv:132-141 taps.  Only (DCT-II, 32) is pinned by upstream.
 * d_offsets == NULL: block b lives at sample offset b*N*N in both buffers.
 * d_offsets != NULL: block b lives at sample offset d_offsets[b] (a multiple of 8) in
 * both buffers -- the per-CTU mixed batches: one call per (type, size) class over a
 * shared residual / coefficient buffer pair. */
#define X266_TR_DCT2 0            /* slot 0 (DCT-II) horizontally and vertically */
#define X266_TR_DST7 1            /* slot 1 (DST-VII) horizontally and vertically */
#define X266_TR_DST7_DCT2 2       /* slot 1 horizontally (along rows), slot 0 vertically: N = 4, 8, 16 */
#define X266_TR_DCT2_DST7 3       /* slot 0 horizontally, slot 1 vertically */
/* Alignment in bytes: d_in 16, d_out 16, d_offsets 4. */
int xTransformFwdBatchDev(x266hip_ctx *ctx, int type, int size, const int16_t *d_in, int16_t *d_out,
                          size_t n_blocks, const uint32_t *d_offsets, void *stream);
/* Caller-supplied 1-D transform matrices (the RTL re-uses one datapath for any tap set the same way,
 * src/mkDct32.bsv:132-141, 385-387).  slot 0 / 1 = the "DCT-II" / "DST-VII" slot of the type codes above,
 * size in {4, 8, 16}; m[k*size + n], row k = basis function, int8 (any values: the kernels only need the int8
 * operand images rebuilt); m == NULL restores the built-in matrix.  Affects every entry point of the set --
 * forward, inverse (which applies the transposes, columns first), the per-class and the one-launch calls, and the CTU calls on
 * tiled frames xTransformCtuFromTilesDev / xTransformCtuToTilesDev -- of THIS context from the next call on.  Synchronises the device (launches in flight read the old tables);
 * not to be called concurrently with other calls on the context.  The 32-point DCT-II cannot be replaced. */
int xTransformSetMatrix(x266hip_ctx *ctx, int slot, int size, const int8_t *m);
int xTransformGetMatrix(const x266hip_ctx *ctx, int slot, int size, int8_t *m);
/* Named contents of slot 1 at all three sizes at once (slot 0 stays the DCT-II), through the same mechanism and with the
 * same all-or-nothing behaviour as xTransformSetMatrix:
 *   X266_PRESET_CLOSED_FORM  the built-in closed-form DST-VII (what a fresh context has)
 *   X266_PRESET_VTM_DST7     H.266's DST-VII integers as recalled from the VTM sources (DEFINE_DST7_P8/P16_MATRIX; N = 4 is the
 *                            closed form) -- marked "as recalled, unverified offline": the build environment holds neither the
 *                            standard nor VTM; a host that has the normative tables should install them with xTransformSetMatrix
 *   X266_PRESET_VTM_DCT8     DCT-VIII, H.266's third MTS kernel, as the flipped, sign-alternated DST-VII of the preset above:
 *                            T8[k][n] = (-1)^k T7[k][N-1-n]; with it the type codes X266_TR_DST7* mean DCT-VIII
 * xTransformPreset returns the preset slot 1 holds, or -1 after xTransformSetMatrix on slot 1. */
#define X266_PRESET_CLOSED_FORM 0
#define X266_PRESET_VTM_DST7    1
#define X266_PRESET_VTM_DCT8    2
int xTransformUsePreset(x266hip_ctx *ctx, int preset);
int xTransformPreset(const x266hip_ctx *ctx);
/* Inverse transforms of the same set (no upstream counterpart): columns first, shifts 7 and 12
 * (8-bit video), int16 clipping after each pass; (DCT-II, 32) contiguous is xDct32InvBatchDev.
 * d_offsets as in the forward call. */
/* Alignment in bytes: d_in 16, d_out 16, d_offsets 4. */
int xTransformInvBatchDev(x266hip_ctx *ctx, int type, int size, const int16_t *d_in, int16_t *d_out,
                          size_t n_blocks, const uint32_t *d_offsets, void *stream);
/* The whole mixed set in ONE launch (BASELINE configs[3], "batched per CTU").  The buffers are sequences of
 * 32x32-sample regions ("tiles", 1024 samples); tile t is cut into (32/N)^2 blocks of one (type, size) class,
 * stored block-major, its class given by d_tile_class[t] = X266_TILE_CLASS(type, size) and its position by
 * d_tile_offsets[t] (sample offset, a multiple of 8; NULL: tile t at t * 1024, i.e. the buffer is the tiles
 * in order -- a CTU-ordered residual buffer whose 64x64 CTUs are four such tiles).  inverse = 0 forward,
 * 1 inverse; results identical to the per-class calls above. */
#define X266_TILE_CLASS(type, size) ((uint8_t)((type) * 4 + ((size) == 4 ? 0 : (size) == 8 ? 1 : (size) == 16 ? 2 : 3)))
/* Alignment in bytes: d_in 16, d_out 16, d_tile_offsets 4, d_tile_class 1. */
int xTransformTilesDev(x266hip_ctx *ctx, int inverse, const int16_t *d_in, int16_t *d_out, size_t n_tiles,
                       const uint32_t *d_tile_offsets, const uint8_t *d_tile_class, void *stream);
/* Full-search motion estimation with the 8x8 SATD cost (BASELINE configs[2]).
 * For every 8x8 block of `cur` (block grid aligned to (0,0); width, height
 * multiples of 8) and every displacement (dx,dy) in [-range, range]^2,
 *     cost = satd8x8(cur_block - ref_block_at(x+dx, y+dy))      (src_tb/satd.c:31-118)
 * and d_best[by * (width/8) + bx] receives the minimum; among equal costs the
 * first candidate in raster order (dy ascending, then dx ascending) wins.
 * `ref` points at pixel (0,0) of a frame padded by at least `range` pixels on
 * every side (rows are ref_stride bytes apart; negative offsets are read).
 * 1 <= range <= 64.  d_costs may be NULL; otherwise it receives every cost,
 * d_costs[block * (2*range+1)^2 + (dy+range)*(2*range+1) + (dx+range)].
 * Strides follow src/x266.cpp:419 (intptr_t, in bytes).  d_cur and d_ref need no alignment and the strides no multiple;
 * d_best is 8-byte and d_costs 4-byte aligned. */
typedef struct x266_me_result_t {
    int16_t  mvx, mvy;      /* best displacement */
    uint32_t cost;          /* its SATD          */
} x266_me_result_t;
/* Alignment in bytes: d_cur 1, d_ref 1, d_best 8, d_costs 4. */
int xSatd8x8SearchDev(x266hip_ctx *ctx, const uint8_t *d_cur, intptr_t cur_stride,
                      const uint8_t *d_ref, intptr_t ref_stride, int width, int height,
                      int range, x266_me_result_t *d_best, uint32_t *d_costs, void *stream);
/* The same search with the cheaper metric: cost = sum |cur - ref| over the 8x8 block,
 * i.e. sad() of riscv/programs/benchmarks/sad/sad.c:28-39 at n = 8; same candidate order and
 * tie-break.  d_cur must be 4-byte aligned with cur_stride a multiple of 4; d_ref, d_best and d_costs as above. */
/* Allocates xSatd8x8SearchDev's scratch (128 bytes per 8x8 block of the frame) for searches of frames up to
 * width x height enqueued on `stream`, so that no launch path allocates: for stream captures and real-time loops.
 * The library keeps one buffer per stream, for at most 8 streams (the least recently used one is released after
 * its last search has finished); buffers handed out under a capture live as long as the context. */
int xHipMeScratchReserve(x266hip_ctx *ctx, void *stream, int width, int height);
/* Alignment in bytes: d_cur 4, d_ref 1, d_best 8, d_costs 4. */
int xSad8x8SearchDev(x266hip_ctx *ctx, const uint8_t *d_cur, intptr_t cur_stride, const uint8_t *d_ref,
                     intptr_t ref_stride, int width, int height, int range, x266_me_result_t *d_best,
                     uint32_t *d_costs, void *stream);
/* Frame container of the codec skeleton: ref_block_t, src/x266.cpp:56-63 -- a frame is a
 * raster of 512-byte tiles (16x16 luma, 8 rows of interleaved U,V pairs, 128 info bytes). */
typedef struct x266_ref_block_t {
    uint8_t m_Y[16 * 16];
    uint8_t m_C[2 * 8 * 8];
    uint8_t m_I[128];
} x266_ref_block_t;
/* xConvInputFmt (src/x266.cpp:415-453) on the device: planar YUV 4:2:0 -> tiles.  width and
 * height multiples of 16; chroma stride = strdY / 2 as upstream; rows 16-byte (luma) and
 * 8-byte (chroma) aligned.  m_I is left untouched, as upstream leaves it. */
/* Alignment in bytes: d_tiles 16, d_y 16, d_u 8, d_v 8. */
int xConvInputFmtDev(x266hip_ctx *ctx, x266_ref_block_t *d_tiles, const uint8_t *d_y, const uint8_t *d_u,
                     const uint8_t *d_v, intptr_t strdY, int width, int height, void *stream);
/* xConvOutput420 (src/x266.cpp:455-492) on the device: tiles -> planar YUV 4:2:0. */
/* Alignment in bytes: d_tiles 16, d_y 16, d_u 8, d_v 8. */
int xConvOutput420Dev(x266hip_ctx *ctx, const x266_ref_block_t *d_tiles, uint8_t *d_y, intptr_t strdY,
                      uint8_t *d_u, uint8_t *d_v, intptr_t strdC, int width, int height, void *stream);
/* Residual formation (no upstream counterpart: upstream stops before the residual stage):
 * luma of two tiled frames, residual = cur - pred as int16, emitted as row-major blocks in
 * raster order of blocks -- block_edge 32 feeds xDct32FwdBatchDev (width, height multiples
 * of 32), block_edge 8 feeds xSatd8x8BatchDev (multiples of 16). */
/* Alignment in bytes: d_cur 16, d_pred 16, d_residual 16. */
int xResidualLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                     int width, int height, int block_edge, int16_t *d_residual, void *stream);
/* Fused residual formation + forward DCT32: d_coef[block] = DCT32(cur - pred) for every 32x32 luma
 * block of two tiled frames, blocks in raster order -- bit-identical to xResidualLumaDev(.., 32, ..)
 * followed by xDct32FwdBatchDev, without the residual ever touching HBM (half the traffic). */
/* Alignment in bytes: d_cur 16, d_pred 16, d_coef 16. */
int xDct32FwdFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                          int width, int height, int16_t *d_coef, void *stream);
/* Fused residual formation + SATD: d_out[block] = satd8x8(cur - pred) for every 8x8 luma block of
 * two tiled frames (raster order of blocks) -- bit-identical to xResidualLumaDev(.., 8, ..) followed
 * by xSatd8x8BatchDev.  width, height multiples of 16. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_out 4. */
int xSatd8x8FromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                         int width, int height, uint32_t *d_out, void *stream);
/* The chroma half of the same stage.  A tile's chroma is m_C (src/x266.cpp:60): 8 rows of 8 interleaved (U, V) pairs, as
 * xConvInputFmt packs them (src/x266.cpp:441-449); the chroma planes of a width x height (luma) 4:2:0 frame are
 * (width / 2) x (height / 2).  block_edge 8: one 8x8 U and one 8x8 V block per tile (width, height multiples of 16),
 * the inputs of xSatd8x8BatchDev; block_edge 32: one 32x32 U and one 32x32 V block per 64x64 CTU (multiples of 64), the
 * inputs of xDct32FwdBatchDev.  Blocks are row-major int16, numbered in raster order within the chroma plane; block b of
 * U goes to d_res_u + b * block_pitch * edge^2, of V to d_res_v + b * block_pitch * edge^2 (block_pitch >= 1, in blocks):
 * block_pitch 1 with two buffers gives two planar block streams, block_pitch 2 with d_res_v = d_res_u + edge^2 gives
 * the CTU-ordered stream U0 V0 U1 V1 ...  (No upstream counterpart, as for luma.) */
/* Alignment in bytes: d_cur 16, d_pred 16, d_res_u 16, d_res_v 16. */
int xResidualChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                       int width, int height, int block_edge, int16_t *d_res_u, int16_t *d_res_v,
                       size_t block_pitch, void *stream);
/* Fused chroma residual + forward DCT32: both 32x32 chroma blocks of every 64x64 CTU, one wave per CTU -- bit-identical to
 * xResidualChromaDev(.., 32, ..) followed by xDct32FwdBatchDev; coefficients of CTU b's U block at
 * d_coef_u + b * block_pitch * 1024, V likewise.  width, height multiples of 64. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_coef_u 16, d_coef_v 16. */
int xDct32FwdChromaFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                                int width, int height, int16_t *d_coef_u, int16_t *d_coef_v, size_t block_pitch,
                                void *stream);
/* A whole 4:2:0 CTU per unit of output, one launch: for every 64x64 CTU (raster order) 12 KiB of coefficients
 * d_coef[ctu * 6144 + q * 1024 ..]: q = 0..3 the forward DCT32 of its four 32x32 luma residual quadrants (top-left, top-right,
 * bottom-left, bottom-right), q = 4 of its 32x32 U residual, q = 5 of V -- bit-identical to xDct32FwdFromTilesDev and
 * xDct32FwdChromaFromTilesDev, whose frame-raster luma and separate chroma streams it re-orders into the order a per-CTU
 * encoder loop consumes (BASELINE configs[3]: "batched per-CTU").  width, height multiples of 64. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_coef 16. */
int xDct32FwdCtuFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                             int width, int height, int16_t *d_coef, void *stream);
/* Fused chroma residual + SATD: d_out_u[t * pitch] = satd8x8 of tile t's U residual, d_out_v[t * pitch] of its V residual
 * (tiles in raster order) -- bit-identical to xResidualChromaDev(.., 8, ..) followed by xSatd8x8BatchDev.  pitch 2 with
 * d_out_v = d_out_u + 1 interleaves the two costs.  width, height multiples of 16. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_out_u 4, d_out_v 4. */
int xSatd8x8ChromaFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                               int width, int height, uint32_t *d_out_u, uint32_t *d_out_v, size_t pitch, void *stream);
/* Reconstruction into tiles, the way back from the stage above (no upstream counterpart, as for residual formation):
 * recon = clamp(pred + residual, 0, 255) per sample, computed exactly for every int16 residual (pred 100 + 32767 gives 255),
 * written into the tiled frame d_recon.  Luma calls write only m_Y and chroma calls only m_C of d_recon, so a luma call and
 * a chroma call compose into one frame; no call writes m_I (as xConvInputFmtDev).  d_recon == d_pred is allowed (an encoder
 * reconstructs over its prediction); any other overlap of d_recon with an input returns X266HIP_EINVAL.  Buffers 16-byte
 * aligned.
 * Luma: the mirror of xResidualLumaDev -- d_residual holds int16 row-major blocks in raster order of blocks, exactly the
 * layout xResidualLumaDev emits; block_edge 32 (width, height multiples of 32) or 8 (multiples of 16).
 * xResidualLumaDev(cur, pred) followed by xReconLumaDev(pred, ..) gives back cur's m_Y. */
/* Alignment in bytes: d_pred 16, d_residual 16, d_recon 16. */
int xReconLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_pred, const int16_t *d_residual, int width, int height,
                  int block_edge, x266_ref_block_t *d_recon, void *stream);
/* Chroma: the mirror of xResidualChromaDev -- the same U / V block streams, block_edge and block_pitch conventions (block b
 * of U at d_res_u + b * block_pitch * edge^2; block_pitch 2 with d_res_v = d_res_u + edge^2 is the CTU-interleaved stream);
 * writes the interleaved (U, V) pairs of m_C (src/x266.cpp:441-449, as xConvInputFmtDev packs them).  block_edge 8: width,
 * height multiples of 16; 32: multiples of 64.  A block_pitch of 0, or one whose stream would not fit in the address space,
 * returns X266HIP_EINVAL. */
/* Alignment in bytes: d_pred 16, d_res_u 16, d_res_v 16, d_recon 16. */
int xReconChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_pred, const int16_t *d_res_u, const int16_t *d_res_v,
                    size_t block_pitch, int width, int height, int block_edge, x266_ref_block_t *d_recon, void *stream);
/* Fused inverse DCT32 + reconstruction: m_Y of d_recon = clamp(pred + IDCT32(coef), 0, 255) for every 32x32 luma block,
 * coefficients in frame raster order of blocks (the order xDct32FwdFromTilesDev emits) -- bit-identical to
 * xDct32InvBatchDev followed by xReconLumaDev(.., 32, ..), without the residual touching HBM (4 KiB moved per block
 * instead of 8).  width, height multiples of 32. */
/* Alignment in bytes: d_coef 16, d_pred 16, d_recon 16. */
int xDct32InvToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const x266_ref_block_t *d_pred, int width, int height,
                        x266_ref_block_t *d_recon, void *stream);
/* The inverse of xDct32FwdCtuFromTilesDev: input 12 KiB per 64x64 CTU (Y0 Y1 Y2 Y3 U V, CTUs in raster order); one launch
 * writes m_Y and m_C of every CTU's 16 tiles -- bit-identical to xDct32InvBatchDev of the six blocks followed by
 * xReconLumaDev(.., 32, ..) and xReconChromaDev(.., 32, ..).  width, height multiples of 64. */
/* Alignment in bytes: d_coef 16, d_pred 16, d_recon 16. */
int xDct32InvCtuToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const x266_ref_block_t *d_pred, int width, int height,
                           x266_ref_block_t *d_recon, void *stream);
/* The mixed transform set (xTransformTilesDev) per CTU, straight from and into tiled frames of any size.
 * Frame: width, height positive multiples of 16; ceil(width / 64) x ceil(height / 64) CTUs of 64x64 in raster order, the right
 * and bottom ones possibly cut by the frame edge.  Each CTU has six 32x32 regions q = 0..5: q = 0..3 its luma quadrants
 * (top-left, top-right, bottom-left, bottom-right), q = 4 its 32x32 U and q = 5 its 32x32 V samples (m_C of its 4x4 tiles) --
 * the order and the 12 KiB-per-CTU layout of xDct32FwdCtuFromTilesDev.  Region q of CTU b has the class d_class[6b + q],
 * read as xTransformTilesDev reads its class bytes (X266_TILE_CLASS(type, size), low four bits; size 32 is always the 32-point
 * DCT-II) and cut into (32/N)^2 blocks of N x N, block-major, blocks in raster order inside the region: xTransformTilesDev's
 * tile layout, so the forward call's d_coef is the input of xTransformTilesDev(1, .., d_class) or of xTransformCtuToTilesDev.
 * Frame edge: samples outside the frame count as residual 0 forward, their inverse outputs are discarded.  A region wholly
 * outside the frame (Y2 / Y3 of the last CTU row at 4320p) gets all-zero coefficients; its slot is still written.  A class
 * whose N divides the region's in-frame extent keeps every block wholly inside or wholly outside the frame -- luma N <= 16 on
 * the 16-row / 16-column strips, chroma N <= 16 on 16-row and N <= 8 on 8- and 24-row strips, the classes an encoder uses
 * there; larger classes give defined output too, and no class byte is checked.
 * Forward: d_coef[b * 6144 + q * 1024 ..] for every region of every CTU (12 KiB per CTU), bit-identical to forming the
 * CTU-ordered residual cur - pred (int16, zero outside the frame, block-major per region class) and running
 * xTransformTilesDev(0, .., d_class) on it.  Inverse: m_Y and m_C of d_recon = clamp(pred + inverse_class(coef), 0, 255) at
 * every in-frame sample, exact for every int16 coefficient (the set's int16 clipping after each pass); m_I is never written.
 * With every class (DCT-II, 32) on a frame whose sides are multiples of 64 the two calls are bit-identical to
 * xDct32FwdCtuFromTilesDev and xDct32InvCtuToTilesDev.
 * Tile and coefficient buffers 16-byte aligned, d_class any alignment.  X266HIP_EINVAL for a bad size, a NULL or unaligned buffer,
 * a buffer whose span does not fit in the address space, or an output overlapping an input -- d_recon == d_pred is allowed, as
 * in the recon calls, and so is d_cur == d_pred (both read-only); X266HIP_EDEVICE when the context's transform tables are
 * invalid.  Neither call allocates: both can be captured into a graph. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_class 1, d_coef 16. */
int xTransformCtuFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred,
                              int width, int height, const uint8_t *d_class, int16_t *d_coef, void *stream);
/* Alignment in bytes: d_coef 16, d_class 1, d_pred 16, d_recon 16. */
int xTransformCtuToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const uint8_t *d_class,
                            const x266_ref_block_t *d_pred, int width, int height,
                            x266_ref_block_t *d_recon, void *stream);
/* Quantisation (no upstream counterpart: SURVEY, "No residual, transform, quant, or entropy stage exists").  The flat scalar
 * quantiser of HEVC / VVC at 8-bit depth, without scaling lists or dependent quantisation, matched to the transforms of this
 * library (forward shifts log2N - 1 and log2N + 6, inverse shifts 7 and 12) -- the constants as recalled, unverified offline
 * (like the DST-VII presets and the chroma filter); the arithmetic here is the contract, not a standard text.  For an N x N
 * block with n = log2 N in 2..5, qp in 0..51 and rounding in 0..511 (units of 1/512; 171 is a third, 256 a half):
 *   f[6] = {26214, 23302, 20560, 18396, 16384, 14564}      g[6] = {40, 45, 51, 57, 64, 72}
 *   qbits = 14 + qp/6 + (7 - n)
 *   level = sign(c) * ((|c| * f[qp%6] + (rounding << (qbits - 9))) >> qbits)
 *   coef' = clip_int16((level * (g[qp%6] << (qp/6)) + (1 << (n - 2))) >> (n - 1))       (arithmetic shift)
 * What follows: qbits >= 16, so qbits - 9 >= 7; |c| <= 32768 gives |level| <= 13108, so the forward direction needs no clip;
 * |c| * f + offset < 2^30 and |level| * (g << qp/6) < 2^30 for every int16 level, so 32-bit arithmetic is exact (and both
 * products fit the 24-bit multiply-add); the dequantiser does need its clip: level 13107 at qp 0, n = 5 rounds to 32768.
 * Example: c = 1000, n = 5, qp = 22, rounding = 171 gives level 31 and coef' 992; c = -1000 gives -31 and -992.
 *
 * xQuantRegionsGpu: d_in and d_out are sequences of n_regions regions of 1024 samples (the unit of xTransformTilesDev and of the
 * 12 KiB-per-CTU layouts, six regions per CTU).  Region r has the block size N of its class byte d_class[r], read as
 * xTransformTilesDev reads its class bytes (low bits: n = 2 + (class & 3)); d_class == NULL means every region is 32x32, which
 * also covers a plain DCT32 batch with n_regions = n_blocks.  N is uniform per region, so the block-major layout inside a region
 * does not matter: the operation is element-wise.  Region r uses min(d_qp[r], 51) when d_qp != NULL (a caller's own chroma qp
 * mapping goes into the bytes of regions 4 and 5 of a CTU), otherwise the scalar qp.  inverse = 0: coefficients -> levels, and
 * d_nnz[r], if d_nnz != NULL, receives the number of non-zero levels of region r (the coded-block flag).  inverse = 1: levels
 * -> coefficients; d_nnz must be NULL.  d_out == d_in (in place) is allowed; any other overlap returns X266HIP_EINVAL.
 * The sample buffers d_in and d_out are 16-byte aligned, d_nnz is 4-byte aligned, d_class and d_qp need no alignment.
 * X266HIP_EINVAL for a NULL or misaligned buffer, a scalar qp outside 0..51 when d_qp == NULL, rounding outside 0..511, or a
 * span that does not fit in the address space.  n_regions == 0 returns 0 and launches nothing.  The call allocates nothing and
 * can be captured into a graph. */
/* Alignment in bytes: d_in 16, d_out 16, d_class 1, d_qp 1, d_nnz 4. */
int xQuantRegionsGpu(x266hip_ctx *ctx, int inverse, const int16_t *d_in, int16_t *d_out, size_t n_regions,
                     const uint8_t *d_class, const uint8_t *d_qp, int qp, int rounding, uint32_t *d_nnz, void *stream);
/* The coding loop of a frame in one launch.  width, height multiples of 64.  For every 64x64 CTU in raster order and its six
 * 32x32 regions q = 0..5 (Y0 Y1 Y2 Y3 U V, as xDct32FwdCtuFromTilesDev): d_level[ctu * 6144 + q * 1024 ..] = Q(DCT32(cur - pred)),
 * d_nnz[6 ctu + q] = its number of non-zero levels (d_nnz may be NULL), and m_Y and m_C of d_recon =
 * clamp(pred + IDCT32(Q^-1(level)), 0, 255); m_I is never written.  Bit-identical to xDct32FwdCtuFromTilesDev ->
 * xQuantRegionsGpu(0) -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev with the same qp arguments (d_qp indexed 6 ctu + q,
 * clamped to 51; NULL: the scalar qp), moving 30 KiB per CTU instead of 96.  d_recon == d_pred and d_cur == d_pred are
 * allowed, as in the calls it fuses; d_level and d_nnz must overlap nothing.
 * The tile buffers d_cur, d_pred, d_recon and the level buffer d_level are 16-byte aligned, d_nnz is 4-byte aligned, d_qp needs
 * no alignment.  X266HIP_EINVAL as for the calls above.  The call allocates nothing and can be captured into a graph. */
/* Alignment in bytes: d_cur 16, d_pred 16, d_qp 1, d_level 16, d_nnz 4, d_recon 16. */
int xDct32CodeCtuTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width,
                          int height, const uint8_t *d_qp, int qp, int rounding, int16_t *d_level, uint32_t *d_nnz,
                          x266_ref_block_t *d_recon, void *stream);
/* Inter prediction on tiled frames (no upstream counterpart: upstream keeps its references as tiled frames, codec_t.m_frames[],
 * src/x266.cpp:96-102, but has no search or compensation for them).  Edge convention of every call below: a reference sample
 * outside the frame takes the nearest in-frame sample, ref[clamp(y, 0, H-1)][clamp(x, 0, W-1)] -- edge replication on all four
 * sides, defined for any displacement, a range larger than the frame included.  width, height multiples of 16; tile buffers
 * 16-byte aligned; records 8-byte aligned, cost maps 4-byte aligned.
 * The searches: xSatd8x8SearchDev / xSad8x8SearchDev (same cost per candidate, candidate order, tie-break, d_best and d_costs
 * layouts, 1 <= range <= 64) with cur and ref the m_Y planes of two tiled frames -- bit-identical to the planar calls on
 * np.pad(ref_plane, range, mode="edge").  d_cur == d_ref is allowed (both are read-only); d_best or d_costs overlapping either
 * frame, or a cost map whose size does not fit in the address space, returns X266HIP_EINVAL.  The SATD form uses the same
 * per-stream scratch as xSatd8x8SearchDev: under a stream capture call xHipMeScratchReserve first (or run one search on that
 * stream beforehand). */
/* Alignment in bytes: d_cur 16, d_ref 16, d_best 8, d_costs 4. */
int xSatd8x8SearchFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref,
                               int width, int height, int range, x266_me_result_t *d_best, uint32_t *d_costs,
                               void *stream);
/* Alignment in bytes: d_cur 16, d_ref 16, d_best 8, d_costs 4. */
int xSad8x8SearchFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref,
                              int width, int height, int range, x266_me_result_t *d_best, uint32_t *d_costs,
                              void *stream);
/* Integer-pel luma motion compensation: one x266_me_result_t per 8x8 block in raster order of blocks (exactly the searches'
 * d_best; cost is ignored), pred[8by+y][8bx+x] = ref[clamp(8by+y+mvy, 0, H-1)][clamp(8bx+x+mvx, 0, W-1)] for any int16 vector.
 * Writes only m_Y of d_pred; m_C and m_I are left untouched, as xReconLumaDev leaves them.  Blocks read what other blocks
 * would overwrite, so d_pred overlapping d_ref or d_mv returns X266HIP_EINVAL. */
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                       int width, int height, x266_ref_block_t *d_pred, void *stream);
/* 4:2:0 chroma motion compensation with the same records: the vector of 8x8 luma block (bx, by) moves the 4x4 block (bx, by) of
 * U and of V (chroma samples 4bx..4bx+3, 4by..4by+3 of the CW x CH = W/2 x H/2 planes) by half of it.  The filter is the
 * half-sample chroma filter of HEVC / VVC, T = (-4, 36, 36, -4), at 8-bit depth -- as recalled, unverified offline (like the
 * DST-VII presets); the arithmetic here is the contract, not a standard text.  For any int16 vector
 *   ix = mvx >> 1, fx = mvx & 1, iy = mvy >> 1, fy = mvy & 1    (arithmetic shift: -1 -> ix = -1, fx = 1),
 *   S(y, x) = plane[clamp(y, 0, CH-1)][clamp(x, 0, CW-1)]       (the inter stage's edge rule, on the chroma plane),
 * and for chroma sample (x, y) of either plane, with clip8 the clamp to 0..255:
 *   fx = 0, fy = 0:  out = S(y+iy, x+ix)                                                   (a pure gather)
 *   fx = 1, fy = 0:  out = clip8((sum_k T[k] * S(y+iy, x+ix+k-1) + 32) >> 6),  k = 0..3
 *   fx = 0, fy = 1:  out = clip8((sum_k T[k] * S(y+iy+k-1, x+ix) + 32) >> 6)
 *   fx = 1, fy = 1:  h(r) = sum_k T[k] * S(r, x+ix+k-1)          (no shift; -2040..18360)
 *                    v = (sum_k T[k] * h(y+iy+k-1)) >> 6         (arithmetic: floors a negative sum)
 *                    out = clip8((v + 32) >> 6)
 * So a zero vector copies m_C, even vectors move bytes unchanged, and a constant plane stays constant for every vector.
 * xMotionCompChromaDev writes only m_C of d_pred (both planes) and leaves m_Y and m_I untouched: after it and
 * xMotionCompLumaDev d_pred is a whole 4:2:0 prediction.  xMotionCompDev writes m_Y and m_C in one launch, bit-identical to the
 * luma call followed by the chroma call; m_I is never written.  Arguments as for xMotionCompLumaDev; neither call allocates,
 * both can be captured into a graph. */
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                         int width, int height, x266_ref_block_t *d_pred, void *stream);
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                   int width, int height, x266_ref_block_t *d_pred, void *stream);
/* Quarter-sample inter prediction: the calls above stop at whole luma samples, the four below predict at the quarter-sample luma
 * (eighth-sample 4:2:0 chroma) precision of HEVC / VVC.  The filter constants are HEVC's as recalled, unverified offline (like
 * the half-sample chroma filter above); the arithmetic here is the contract, not a standard text.  The same tap row serves both axes.
 *   luma, 8 taps, tap k at offset k - 3:    TL[0] = { 0, 0,   0, 64,  0,   0, 0,  0}    TL[1] = {-1, 4, -10, 58, 17,  -5, 1,  0}
 *                                           TL[2] = {-1, 4, -11, 40, 40, -11, 4, -1}    TL[3] = { 0, 1,  -5, 17, 58, -10, 4, -1}
 *   chroma, 4 taps, tap k at offset k - 1:  TC[0] = { 0, 64,  0,  0}  TC[1] = {-2, 58, 10, -2}  TC[2] = {-4, 54, 16, -2}
 *       TC[3] = {-6, 46, 28, -4}  TC[4] = {-4, 36, 36, -4}  TC[5] = {-4, 28, 46, -6}  TC[6] = {-2, 16, 54, -4}  TC[7] = {-2, 10, 58, -2}
 * The records are x266_me_result_t in QUARTER luma samples, one per 8x8 luma block in raster order of blocks; the vector of luma
 * block (bx, by) also moves the 4x4 U and V blocks (bx, by), as in xMotionCompChromaDev.  Luma uses T = TL, lg = 2, o = 3 on the luma
 * plane, chroma T = TC, lg = 3, o = 1 on each chroma plane; S(y, x) = plane[clamp(y, 0, H-1)][clamp(x, 0, W-1)] is the inter stage's
 * edge rule on that plane.  For any int16 vector (arithmetic shifts: -1 has integer part -1 and fraction 2^lg - 1)
 *   ix = mvx >> lg, fx = mvx & (2^lg - 1), iy = mvy >> lg, fy = mvy & (2^lg - 1)
 *   fx = 0, fy = 0:  out = S(y+iy, x+ix)
 *   fy = 0:          out = clip8((sum_k T[fx][k] * S(y+iy, x+ix+k-o) + 32) >> 6)
 *   fx = 0:          out = clip8((sum_k T[fy][k] * S(y+iy+k-o, x+ix) + 32) >> 6)
 *   otherwise:       h(r) = sum_k T[fx][k] * S(r, x+ix+k-o)         (no shift; luma -6120..22440, fits int16)
 *                    v = (sum_k T[fy][k] * h(y+iy+k-o)) >> 6        (32-bit sum; arithmetic: floors a negative sum)
 *                    out = clip8((v + 32) >> 6)
 * The horizontal stage is unshifted, so v comes from the exact double sum and the order of the two passes does not matter.
 * What follows: a vector 4m reproduces xMotionCompLumaDev and xMotionCompChromaDev with vector m bit for bit, for |m| <= 8191
 * (chroma phase 4 is the (-4, 36, 36, -4) of that call); a constant plane stays constant for every vector.
 * xMotionCompQpelLumaGpu writes only m_Y of d_pred, xMotionCompQpelChromaGpu only m_C, xMotionCompQpelGpu both in one launch,
 * bit-identical to the pair; m_I is never read or written.  Arguments as for the three integer calls: width, height multiples of 16,
 * d_ref and d_pred 16-byte aligned, d_mv 8-byte aligned; X266HIP_EINVAL for a NULL or misaligned pointer, a bad size, a buffer whose
 * span does not fit in the address space, or d_pred overlapping d_ref or d_mv.  Nothing is allocated; the calls can be captured
 * into a graph.  Tile offsets are size_t as in the integer calls, but frames beyond 2^32 bytes are untested for these four calls. */
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompQpelLumaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                           int width, int height, x266_ref_block_t *d_pred, void *stream);
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompQpelChromaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                             int width, int height, x266_ref_block_t *d_pred, void *stream);
/* Alignment in bytes: d_ref 16, d_mv 8, d_pred 16. */
int xMotionCompQpelGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                       int width, int height, x266_ref_block_t *d_pred, void *stream);
/* Quarter-sample refinement of integer vectors.  d_int holds one integer record per 8x8 luma block (the searches' d_best; its cost
 * is ignored).  For block b, m = clamp(mv_int, -8191, 8191) per component, so that every candidate fits int16; the 49 candidates
 * are q = 4m + (dx, dy), dx, dy in -3..3, and cost(q) = satd8x8(cur_block - P_q) with P_q the block's 8x8 luma prediction of
 * xMotionCompQpelLumaGpu under q and satd8x8 the metric of the searches (src_tb/satd.c:31-118).  d_best[b] = the candidate of least
 * cost, in quarter samples, with its cost; among equal costs (0, 0) wins, after it the first in raster order (dy ascending, then dx
 * ascending).  d_costs may be NULL; otherwise d_costs[49 b + 7 (dy + 3) + (dx + 3)] receives every cost, so its centre entry is the
 * integer search's cost of m.  d_best == d_int (in place) and d_cur == d_ref are allowed; any other overlap of d_best or d_costs
 * with anything returns X266HIP_EINVAL.  d_cur and d_ref are 16-byte aligned, d_int and d_best 8-byte, d_costs 4-byte; other
 * arguments and errors as above.  No per-stream scratch is used (unlike the SATD search): the call allocates nothing, needs no
 * xHipMeScratchReserve and can be captured into a graph. */
/* Alignment in bytes: d_cur 16, d_ref 16, d_int 8, d_best 8, d_costs 4. */
int xSatd8x8RefineQpelFromTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref,
                                   int width, int height, const x266_me_result_t *d_int, x266_me_result_t *d_best,
                                   uint32_t *d_costs, void *stream);
/* Bi-directional inter prediction: a block predicted from TWO references (list 0 and list 1), one quarter-sample vector each,
 * averaged at the intermediate precision, with explicit weights for fades.  8-bit 4:2:0 on tiled frames with the inter stage's
 * edge rule; the filters, TL / TC, lg, o and the vector split are those of the quarter-sample calls above (the constants as
 * recalled, unverified offline; the arithmetic here is the contract).
 * Intermediate.  For one plane, one reference and one quarter-sample vector, with h the unshifted horizontal sum,
 *   V(y, x) = (sum_k T[fy][k] * h(y + iy + k - o)) >> 6        (arithmetic shift)
 * for all four phase classes alike: phase 0 multiplies by 64, so an integer vector gives V = 64 S, and the prediction of the uni
 * calls above is clip8((V + 32) >> 6).  Luma V lies in -16830..33150 (both reached at phase (2, 2) on a 0 / 255 pattern that
 * follows the sign of TL[2][k] * TL[2][j]) and chroma V in -5897..22217 (the largest value reached is 22216): V does NOT fit int16.
 * Weights.  w and o are indexed [list][Y, U, V], log2_denom [luma, chroma]; w and o are -128..127, log2_denom 0..7.  The struct is
 * read on the host at call time and passed by value into the launch: a captured graph replays the values it was captured with.
 * wp == NULL means default weights.  With D = log2_denom + 6:
 *   uni, list l:  clip8(((V_l * w_l + (1 << (D - 1))) >> D) + o_l)
 *   bi:           clip8((V0 * w0 + V1 * w1 + ((o0 + o1 + 1) << D)) >> (D + 1))
 *   default:      uni clip8((V + 32) >> 6), bi clip8((V0 + V1 + 64) >> 7)
 * w = 1 << log2_denom with o = 0 reproduces the default for every input: V * 2^d + 2^(d+5) = 2^d (V + 32) and likewise for bi.
 * All sums fit int32: |V * w| < 4.3e6 and the offset term is below 2^21.
 * Pointers: tiles 16-byte aligned, records 8, uint32 outputs 4, direction bytes 1.  width, height positive multiples of 16.
 * Nothing allocates; every call can be captured into a graph.  X266HIP_EINVAL as for the quarter-sample calls (NULL, alignment,
 * size, a span that does not fit in the address space, an output overlapping anything) plus a wp field out of range and the
 * scalars named below. */
typedef struct x266_wp_t {
    int16_t w[2][3];
    int16_t o[2][3];
    uint8_t log2_denom[2];
} x266_wp_t;
/* Motion compensation from two references.  d_dir[b] & 3 is the direction of 8x8 luma block b (raster order): 1 = list 0 only,
 * 2 = list 1 only, 3 = both, 0 = the block's bytes of d_pred are left untouched (an intra block of a B-frame).  d_dir == NULL: every
 * block is 3.  planes: 1 = m_Y, 2 = m_C, 3 = both in one launch, bit-identical to the two single-plane calls; m_I is never written.
 * The luma block's vectors and direction also move its 4x4 U and V blocks.  d_ref0 == d_ref1 is allowed; d_pred must overlap
 * nothing.  Both vector arrays are required whatever d_dir says (an unused record is read and ignored).  With wp == NULL a block
 * of direction 1 is the uni quarter-sample prediction of (d_ref0, d_mv0) bit for bit, direction 2 likewise for list 1. */
/* Alignment in bytes: d_ref0 16, d_ref1 16, d_mv0 8, d_mv1 8, d_dir 1, d_pred 16. */
int xMotionCompBiQpelTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1,
                           const x266_me_result_t *d_mv0, const x266_me_result_t *d_mv1, const uint8_t *d_dir,
                           const x266_wp_t *wp, int planes, int width, int height, x266_ref_block_t *d_pred, void *stream);
/* The per-block choice between list 0, list 1 and both.  d_costs[3 b + k] = satd8x8(cur_block - P_k), P_0, P_1, P_2 the luma
 * predictions of the call above under direction 1, 2, 3; satd8x8 is the metric of the searches.  d_dir[b] = the direction of the
 * least of (c0, c1, c2 + bi_penalty), among equal values the earlier in that order.  bi_penalty is 0..65535, the caller's price for
 * the second vector.  Either output may be NULL, not both; an output must overlap nothing. */
/* Alignment in bytes: d_cur 16, d_ref0 16, d_ref1 16, d_mv0 8, d_mv1 8, d_costs 4, d_dir 1. */
int xSatd8x8BiCostsFromTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref0,
                             const x266_ref_block_t *d_ref1, int width, int height, const x266_me_result_t *d_mv0,
                             const x266_me_result_t *d_mv1, const x266_wp_t *wp, int bi_penalty, uint32_t *d_costs,
                             uint8_t *d_dir, void *stream);
/* Re-refinement of one list's vector with the other list's prediction held fixed.  The geometry of the quarter-sample refinement
 * above: integer records d_int clamped to +-8191, 49 candidates q = 4m + (dx, dy), the same tie rule, the same d_costs[49 b + ...]
 * layout (NULL allowed), d_best == d_int allowed.  cost(q) = satd8x8(cur_block - Bi), Bi the bi formula between the fixed list's V
 * under d_mv_fix[b] (quarter samples, any int16 vector) on d_ref_fix and the candidate's V on d_ref.  list is 0 or 1 and names
 * the list being refined: the candidate takes w[list], o[list], the fixed term the other list's. */
/* Alignment in bytes: d_cur 16, d_ref_fix 16, d_mv_fix 8, d_ref 16, d_int 8, d_best 8, d_costs 4. */
int xSatd8x8RefineBiQpelFromTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref_fix,
                                  const x266_me_result_t *d_mv_fix, const x266_ref_block_t *d_ref,
                                  const x266_me_result_t *d_int, int list, const x266_wp_t *wp, int width, int height,
                                  x266_me_result_t *d_best, uint32_t *d_costs, void *stream);
/* In-loop deblocking of a tiled reconstructed frame (no upstream counterpart, as for the quantiser): HEVC's deblocking filter at
 * 8-bit depth, as recalled, unverified offline; the arithmetic here is the contract, not a standard text.  clip8 = clamp to 0..255,
 * clamp(v, lo, hi) as usual, shifts arithmetic.
 *   BETA[52]: 0 for index < 16, 6..18 in steps of 1 for 16..28, 20..64 in steps of 2 for 29..51
 *   TC[54]:   18 x 0, 9 x 1, 4 x 2, 4 x 3, 3 x 4, 2 x 5, 2 x 6, then 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24
 * Frame: width, height positive multiples of 16; ceil(width / 64) x ceil(height / 64) CTUs, cut CTUs and the region index 6 ctu + q
 * (q = 0..3 the luma quadrants, 4 = U, 5 = V) exactly as in xTransformCtuFromTilesDev; entries of regions wholly outside the frame
 * are never read.  Per region: N = 4 << (class & 3) its block size (d_class NULL: 32), qp = min(d_qp byte, 51) (d_qp NULL: the scalar
 * qp), coded = d_nnz entry != 0 (d_nnz NULL: coded), and for luma quadrants intra = d_intra byte != 0 (d_intra NULL: not intra).
 * Luma.  Edges lie on the 8-sample grid, x = 8k and y = 8m strictly inside the frame (the frame border is never filtered); an edge
 * separates two adjacent 8x8 blocks P (left / above) and Q.  It is a transform edge if P and Q lie in different luma regions or its
 * coordinate inside their common 32x32 region is a multiple of N (for N <= 8: every grid edge).  Boundary strength, first match:
 *   Bs = 2  transform edge and (intra(P) or intra(Q))
 *   Bs = 1  transform edge and (coded(P) or coded(Q))
 *   Bs = 1  neither intra, d_mv != NULL and (|mvxP - mvxQ| >= 4 or |mvyP - mvyQ| >= 4)   (d_mv: quarter luma samples, one record
 *           per 8x8 block in raster order, cost ignored; differences taken in 32 bits)
 *   Bs = 0  otherwise: the edge is left alone.
 *   qP = (qp(P) + qp(Q) + 1) >> 1,  beta = BETA[clamp(qP + 2 beta_offset_div2, 0, 51)],
 *   tc = TC[clamp(qP + 2 (Bs - 1) + 2 tc_offset_div2, 0, 53)]
 * An 8-sample edge is two segments of 4 lines; the samples across the edge on line i are p3 p2 p1 p0 | q0 q1 q2 q3.  Per segment,
 * with i in {0, 3}: dp_i = |p2 - 2 p1 + p0|, dq_i = |q2 - 2 q1 + q0|, d = dp_0 + dq_0 + dp_3 + dq_3; d >= beta: the segment is
 * left alone.  It is strong if for both i: 2 (dp_i + dq_i) < (beta >> 2) and |p3 - p0| + |q0 - q3| < (beta >> 3) and
 * |p0 - q0| < ((5 tc + 1) >> 1).  dEp = (dp_0 + dp_3) < ((beta + (beta >> 1)) >> 3), dEq likewise from dq.
 *   strong, per line, each result clamped to +-2 tc around its input:
 *     p0' = (p2 + 2 p1 + 2 p0 + 2 q0 + q1 + 4) >> 3, p1' = (p2 + p1 + p0 + q0 + 2) >> 2, p2' = (2 p3 + 3 p2 + p1 + p0 + q0 + 4) >> 3,
 *     q0', q1', q2' mirrored
 *   normal, per line: D = (9 (q0 - p0) - 3 (q1 - p1) + 8) >> 4; |D| >= 10 tc: the line is left alone; otherwise D = clamp(D, -tc, tc),
 *     p0' = clip8(p0 + D), q0' = clip8(q0 - D),
 *     if dEp: p1' = clip8(p1 + clamp((((p2 + p0 + 1) >> 1) - p1 + D) >> 1, -(tc >> 1), tc >> 1))
 *     if dEq: q1' = clip8(q1 + clamp((((q2 + q0 + 1) >> 1) - q1 - D) >> 1, -(tc >> 1), tc >> 1))
 * Chroma.  U and V are handled each on its own; edges lie on the 8-chroma-sample grid, i.e. exactly on the tile boundaries, and
 * separate the 8x8 chroma blocks of two adjacent tiles P and Q.  An edge is filtered iff it is a transform edge of that plane (P and Q
 * in different CTUs, or its coordinate in the CTU's 32x32 chroma region is a multiple of the N of region 4 for U, 5 for V) and the luma
 * quadrant containing P's tile or Q's tile is intra.  tc = TC[clamp(((qpC(P) + qpC(Q) + 1) >> 1) + 2 + 2 tc_offset_div2, 0, 53)] with
 * qpC the qp of region 4 (U) or 5 (V) of the tile's CTU: the caller's chroma mapping lives in those bytes, as for the quantiser.
 *   per line: D = clamp((((q0 - p0) << 2) + p1 - q1 + 4) >> 3, -tc, tc), p0' = clip8(p0 + D), q0' = clip8(q0 - D)
 * Order, per plane: all vertical edges of the frame, then all horizontal edges on the result of the first pass.
 * What follows: an edge reads 4 samples (chroma 2) and changes at most 3 (chroma 1) on each side, and decisions use only lines of their
 * own segment; so the 8x8 areas centred on the grid crossings, [8k-4, 8k+4) x [8m-4, 8m+4) clipped at the frame, partition the plane and
 * the whole two-pass result inside such an area depends only on that area's own input samples.  The kernels rely on it: a workgroup
 * reads only what it alone writes, which makes d_out == d_in (in place, the case an encoder uses) legal and the stage one read and one
 * write of the plane.
 * xDeblockLumaGpu writes only m_Y of d_out -- every in-frame sample, filtered or copied --, xDeblockChromaGpu only m_C, xDeblockGpu both
 * in one launch, bit-identical to the pair; m_I is never read or written.  x266_deblock_t is a host struct read during the call; the
 * pointers in it are device pointers.  d_in and d_out are 16-byte aligned, d_mv 8, d_nnz 4, the byte arrays 1.  X266HIP_EINVAL for a NULL
 * p, a NULL or misaligned frame, a misaligned side array, a bad size, qp outside 0..51 when d_qp == NULL, an offset outside -6..6, a span
 * that does not fit in the address space, or d_out overlapping d_in (other than d_out == d_in) or a side array.  The calls allocate
 * nothing and can be captured into a graph. */
typedef struct x266_deblock_t {
    const uint8_t  *d_class;             /* [6 n_ctu] as xTransformCtuFromTilesDev reads it; NULL: every region is (DCT-II, 32) */
    const uint8_t  *d_intra;             /* [6 n_ctu], entries q = 0..3 (luma quadrants) read, non-zero = intra; NULL: none    */
    const uint32_t *d_nnz;               /* [6 n_ctu] as xDct32CodeCtuTilesGpu writes it; NULL: every region counts as coded  */
    const uint8_t  *d_qp;                /* [6 n_ctu], min(.., 51) as xQuantRegionsGpu; NULL: the scalar qp (0..51)            */
    const x266_me_result_t *d_mv;        /* quarter luma samples, one per 8x8 block, raster order; NULL: the motion term never fires */
    int qp, beta_offset_div2, tc_offset_div2;   /* offsets -6..6 */
} x266_deblock_t;
/* Alignment in bytes: d_in 16, d_out 16, d_class 1, d_intra 1, d_nnz 4, d_qp 1, d_mv 8. */
int xDeblockLumaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p,
                    x266_ref_block_t *d_out, void *stream);
/* Alignment in bytes: d_in 16, d_out 16, d_class 1, d_intra 1, d_nnz 4, d_qp 1, d_mv 8. */
int xDeblockChromaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p,
                      x266_ref_block_t *d_out, void *stream);
/* Alignment in bytes: d_in 16, d_out 16, d_class 1, d_intra 1, d_nnz 4, d_qp 1, d_mv 8. */
int xDeblockGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p,
                x266_ref_block_t *d_out, void *stream);
/* Sample adaptive offset (SAO) of a tiled frame, the second in-loop filter (no upstream counterpart, as for the quantiser and the
 * deblocking filter): HEVC's SAO at 8-bit depth, encoder statistics and decision included.  The categories, ranges and rate model
 * are HEVC's as recalled, unverified offline; the arithmetic here is the contract, not a standard text.  clip8 = clamp to 0..255.
 * Frame: width, height positive multiples of 16; ceil(width / 64) x ceil(height / 64) CTUs in raster order, the right and bottom
 * ones cut by the frame exactly as in xTransformCtuFromTilesDev.  Component 0 of CTU t is Y (m_Y, up to 64 x 64 samples), 1 and 2
 * are U and V (the even and odd bytes of m_C, up to 32 x 32 samples each); only in-frame samples exist; m_I is never read or written.
 * Categories.  `dec` is the frame being filtered, `org` the source.  For sample c = dec[y][x] of a PW x PH plane, edge-offset (EO)
 * class k has the neighbours a, b:  k = 0: (x-1, y), (x+1, y);  1: (x, y-1), (x, y+1);  2: (x-1, y-1), (x+1, y+1);
 * 3: (x+1, y-1), (x-1, y+1).  A neighbour outside the plane: category 0 for that class.  A neighbour in another CTU is an ordinary
 * sample of the input frame.  Otherwise s = sign(c - a) + sign(c - b) gives the category: -2 -> 1, -1 -> 2, 0 -> 0, +1 -> 3,
 * +2 -> 4.  The band of a sample is c >> 3 (0..31).
 * Statistics.  d_stats holds per CTU t and component m 48 pairs (count uint32, sum int32), pair e at
 * d_stats[((3 t + m) 48 + e) 2 + {0, 1}] (384 bytes per record): e = 4 k + (cat - 1) for EO class k and category 1..4, e = 16 + band
 * for the bands; count = the CTU's in-frame samples of that component in the bin, sum = the sum of (org - dec) over them.  Every
 * record of every CTU is written (zeros where nothing falls).  |sum| <= 4096 * 255: int32 is exact.
 * Decision.  lambda_q4 in 0..65535 is the Lagrange multiplier in 1/16 of a squared-error unit per bin; all arithmetic is integer.
 *   Offset of a bin (N, E) in [lo, hi]: h0 = clamp(sign(E) ((2 |E| + N) / (2 N)), lo, hi), h0 = 0 if N = 0; the candidates are h0,
 *   each step of 1 towards 0, and 0; J(h) = 16 (N h^2 - 2 h E) + lambda_q4 R(h), R(h) = min(|h| + 1, 7), plus 1 for a band with
 *   h != 0 (its sign); least J wins, among equal costs the smaller |h|.
 *   EO class k: categories 1, 2 use [0, 7], 3, 4 use [-7, 0]; J_EO(k) = the sum of the four least J.
 *   Band offset (BO): every band uses [-7, 7]; position p in 0..28 minimises J_BO(p) = sum_{i<4} J(band p + i), the smallest p first.
 *   Luma, candidates in this order: off, J = lambda_q4;  EO k = 0..3, J = 4 lambda_q4 + J_EO(k);  BO, J = 7 lambda_q4 + J_BO(p).
 *   Chroma: U and V share the type and, for EO, the class (HEVC's syntax); offsets and the band position are per plane.  off,
 *   J = lambda_q4;  EO k, J = 4 lambda_q4 + J_EO^U(k) + J_EO^V(k);  BO, J = 12 lambda_q4 + J_BO^U(p_U) + J_BO^V(p_V).
 *   The candidate of least J wins, among equal costs the first in the order.
 *   32 bits suffice: a CTU component has at most 4096 samples, so over the bins of one class (or over all bands) sum N <= 4096 and
 *   sum |E| <= 4096 * 255; with |h| <= 7, |16 sum (N h^2 - 2 h E)| <= 16 (4096 * 49 + 14 * 4096 * 255) < 2.4e8, the rate terms of
 *   a candidate are at most 65535 * (12 + 8 * 8) < 5.1e6, and a chroma candidate adds two such sums: below 2^31.
 *   Output: one x266_sao_t per CTU and component at d_param[3 t + m]: type 0 off, 1 BO, 2 EO; arg = the EO class or the band
 *   position; off = the offsets of categories 1..4 (EO) or of bands p..p+3 (BO); an off record is all zero; zero[] is written as 0.
 * Apply.  Each sample uses the record of its own CTU and component.  type == 2: out = clip8(c + off[cat - 1]) for category 1..4 of
 * class arg & 3, category 0 copies.  type == 1: j = ((c >> 3) - arg) & 31; j < 4: out = clip8(c + off[j]), otherwise a copy (the
 * position wraps as in the standard, although the decision emits none above 28).  Any other type copies.  Offsets are taken as any
 * int8; no device byte is validated.  Every in-frame sample of m_Y and m_C of d_out is written, filtered or copied.
 * xSaoSearchGpu is xSaoStatsGpu and xSaoDecideGpu in one launch, bit-identical to the pair (the form an encoder uses: the bins need
 * not reach memory); a non-NULL d_stats also receives the statistics.
 * Frames are 16-byte aligned, d_stats 4, d_param 8.  d_org == d_dec is allowed (both are read-only).  Apply reads neighbours that
 * other workgroups write: d_out overlapping d_in in any way, d_out == d_in included, returns X266HIP_EINVAL, as does any output
 * overlapping any other buffer of its call, a NULL or misaligned pointer (only xSaoSearchGpu's d_stats may be NULL), a bad size,
 * lambda_q4 outside 0..65535, n_ctu >= 2^31 or a span that does not fit in the address space.  n_ctu == 0 returns 0 and launches
 * nothing.  Nothing is allocated; every call can be captured into a graph; a refused call launches nothing and names itself in
 * xHipLastError. */
typedef struct x266_sao_t {
    uint8_t type, arg;
    int8_t  off[4];
    uint8_t zero[2];
} x266_sao_t;                            /* 8 bytes */
/* Alignment in bytes: d_org 16, d_dec 16, d_stats 4. */
int xSaoStatsGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height,
                 int32_t *d_stats, void *stream);
/* Alignment in bytes: d_stats 4, d_param 8. */
int xSaoDecideGpu(x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, int lambda_q4, x266_sao_t *d_param, void *stream);
/* Alignment in bytes: d_org 16, d_dec 16, d_param 8, d_stats 4. */
int xSaoSearchGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height,
                  int lambda_q4, x266_sao_t *d_param, int32_t *d_stats, void *stream);
/* Alignment in bytes: d_in 16, d_param 8, d_out 16. */
int xSaoApplyGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_sao_t *d_param,
                 x266_ref_block_t *d_out, void *stream);
/* Adaptive loop filter (ALF) of a tiled frame, the third in-loop filter (no upstream counterpart, as for the quantiser, the deblocking
 * filter and SAO): VVC's ALF at 8-bit depth -- block classification, the clipped diamond filters, the encoder's statistics and a
 * per-CTU decision --, as recalled, unverified offline; the arithmetic here is the contract, not a standard text.  clip8 = clamp to
 * 0..255, clamp(v, lo, hi) as usual, shifts arithmetic.  Out of scope: the virtual boundaries of VVC's line-buffer rule, the 64
 * fixed filter sets, the cross-component filter, the solve that turns statistics into coefficients (it stays on the host:
 * xAlfSumStatsGpu gives it the frame totals), and any coefficient or clip-index rate beyond the per-CTU term of the decision.
 * Planes.  width, height positive multiples of 16; luma is width x height (m_Y), U and V are width / 2 x height / 2 (the even and
 * odd bytes of m_C); ceil(width / 64) x ceil(height / 64) CTUs in raster order, the right and bottom ones cut by the frame exactly
 * as in xSaoStatsGpu; CTU t has up to 64 x 64 luma and 32 x 32 U and V samples.  r(x, y) of a PW x PH plane is the sample at
 * (clamp(x, 0, PW - 1), clamp(y, 0, PH - 1)): every fetch clamps its own coordinates, x and y each on its own (edge replication).
 * A neighbour in another CTU is an ordinary sample of the input frame.  m_I is never read or written.
 * Classification.  Luma only.  One byte per 4x4 block, block (bx, by) at d_class[by (width / 4) + bx]: (width / 4) (height / 4)
 * bytes.  The four sums run over the 32 positions (x, y) with 4 bx - 2 <= x <= 4 bx + 5, 4 by - 2 <= y <= 4 by + 5 and x + y even
 * (the parity of the unclamped coordinates); with c = r(x, y):
 *   V  += |2 c - r(x, y-1) - r(x, y+1)|          H  += |2 c - r(x-1, y) - r(x+1, y)|
 *   D0 += |2 c - r(x-1, y-1) - r(x+1, y+1)|      D1 += |2 c - r(x+1, y-1) - r(x-1, y+1)|
 * Each sum is at most 32 * 510 = 16320, so 32 bits hold every product below.  Then, in this order:
 *   V > H:  (hv1, hv0, dirHV) = (V, H, 1),  otherwise (H, V, 3)
 *   D0 > D1:  (d1, d0, dirD) = (D0, D1, 0),  otherwise (D1, D0, 2)
 *   d1 hv0 > hv1 d0:  (m1, m0, dir1, dir2) = (d1, d0, dirD, dirHV),  otherwise (hv1, hv0, dirHV, dirD)
 *   dirS = 2 if 2 m1 > 9 m0, else 1 if m1 > 2 m0, else 0
 *   act = VAR[min(15, (H + V) >> 5)],  VAR[16] = {0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4}
 *   class = act + (dirS ? 5 (((dir1 & 1) << 1) + dirS) : 0), in 0..24
 *   tr = TT[2 dir1 + (dir2 >> 1)],  TT[8] = {0, 1, 0, 2, 2, 3, 1, 3}
 * The byte is class | tr << 5.  A byte read from a caller's d_class is decoded as class = min(b & 31, 24), tr = (b >> 5) & 3; no
 * device byte is validated.
 * Taps.  Tap i sits at P[i] = (dx, dy) and also covers its mirror (-dx, -dy).  Luma, the 7x7 diamond, 12 taps:
 *   P[0..11] = (0,-3) (-1,-2) (0,-2) (1,-2) (-2,-1) (-1,-1) (0,-1) (1,-1) (2,-1) (-3,0) (-2,0) (-1,0)
 * Chroma, the 5x5 diamond, 6 taps:  P[0..5] = (0,-2) (-1,-1) (0,-1) (1,-1) (-2,0) (-1,0).
 * In a luma block with transposition tr, tap i sits at g_i = G_tr(P[i]): G_0 = (dx, dy), G_1 = (dy, dx), G_2 = (dx, -dy),
 * G_3 = (dy, -dx).  Chroma has no classes and no transposition: g_i = P[i].
 * Filters.  Coefficients are int8 with 7 fractional bits; a clip byte selects K[clip & 3], K[4] = {256, 32, 8, 2}; zero[] is not read.
 * The caller passes device arrays of n_luma (0..8) luma sets -- one filter per class -- and of n_chroma (0..8) chroma alternatives.
 * d_ctrl[3 t + m] is one byte per CTU t and component m (0 = Y, 1 = U, 2 = V): 0 copies; k >= 1 uses luma set k - 1 (m = 0) or
 * chroma alternative k - 1 (m = 1, 2); k above the count copies.
 * Apply.  Per sample c = r(p), with the set, class and transposition of its CTU and 4x4 block (chroma: the alternative of its CTU):
 *   s = sum_i coef[i] (clamp(r(p + g_i) - c, -K_i, K_i) + clamp(r(p - g_i) - c, -K_i, K_i)),   out = clip8(c + ((s + 64) >> 7))
 * |s| <= 12 * 128 * 512: 32 bits suffice.  Every in-frame sample of m_Y and m_C of d_out is written, filtered or copied.  Apply reads
 * neighbours that other workgroups write: d_out overlapping d_in in any way is refused, as for xSaoApplyGpu.
 * Statistics.  `org` is the source, `dec` the frame ALF will filter.  Per sample of dec: y = org - dec and
 * E_i = r(p + g_i) + r(p - g_i) - 2 c, the unclipped tap, so the statistics are those of clip index 0.  Per CTU t the record at
 * d_stats[2358 t] is 2358 int32 (9432 bytes): 25 luma class records of 92 words, then a U and a V record of 29 words.  A record
 * holds, in this order: count; sum y^2; b_i = sum E_i y (12 or 6 words); A_ij = sum E_i E_j for i <= j, the upper triangle row by row
 * (78 or 21 words).  The sums run over the CTU's in-frame samples of that class (luma, each block with its own transposition) or
 * plane.  Every word of every record is written, zeros where nothing falls.  int32 is exact: |A| <= 4096 * 510^2 < 2^31,
 * |b| <= 4096 * 510 * 255, sum y^2 <= 4096 * 255^2.
 * Totals.  xAlfSumStatsGpu adds, word by word, the records of the CTUs whose d_mask byte is non-zero (d_mask NULL: all n_ctu) into
 * the 2358 int64 words of d_total -- what the host downloads to solve for filters.  Integer sums: the result depends on nothing
 * but its inputs.
 * Decision.  The change of a record's squared error under coefficients c, in Q14 (coefficient units squared), read off the statistics:
 *   cost(record, c) = sum_i c_i^2 A_ii + 2 sum_{i<j} c_i c_j A_ij - 256 sum_i c_i b_i
 * Clip indices are ignored: the estimate is exact only for clip index 0 and before the rounding of (s + 64) >> 7.  All arithmetic is
 * int64: whatever int32 words the record holds, a record's cost is below 2^14 * 2^31 * 144 + 2^15 * 2^31 * 12 < 2^53, 25 of them
 * and the rate term (at most 65535 * 2^10 * 3) stay below 2^58.  lambda_q4 in 0..65535 as for SAO; ceil_log2(1) = 0, (2) = 1,
 * (3, 4) = 2, (5..8) = 3.
 *   Luma: J(off) = 0; J(set s) = sum over the 25 classes of cost(class record, coef[class] of set s) + (lambda_q4 << 10) ceil_log2(n_luma).
 *   The least J wins; among equal J, off first, then the smaller s.  d_ctrl[3 t] = 0 for off, s + 1 for set s.
 *   U and V: the same, each on its own record, over the chroma alternatives with ceil_log2(n_chroma), into d_ctrl[3 t + 1], [3 t + 2].
 *   A component whose count is 0 (luma: the sum of the 25 counts) gets 0.
 * With d_class == NULL xAlfStatsGpu and xAlfApplyGpu classify inside, bit-identical to xAlfClassifyGpu followed by the same call on
 * its output.  Frames are 16-byte aligned, d_stats 4, d_total 8, d_luma and d_chroma 4, the byte arrays (d_class, d_mask, d_ctrl) 1.
 * A set array is not looked at, and may be NULL, when its count is 0.  d_org == d_dec is allowed (both are read-only).
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError, for a NULL or misaligned pointer (d_mask, and d_class of
 * the statistics and of apply, may be NULL), a bad size, a count outside 0..8, lambda_q4 outside 0..65535, n_ctu >= 2^31, a span that
 * does not fit in the address space, or an output overlapping any other buffer of its call.  n_ctu == 0 returns 0 and launches
 * nothing (d_total is then left as it was).  Nothing is allocated; every call can be captured into a graph. */
typedef struct x266_alf_luma_t {
    int8_t  coef[25][12];
    uint8_t clip[25][12];
} x266_alf_luma_t;                       /* 600 bytes */
typedef struct x266_alf_chroma_t {
    int8_t  coef[6];
    uint8_t clip[6];
    uint8_t zero[4];
} x266_alf_chroma_t;                     /* 16 bytes */
/* Alignment in bytes: d_dec 16, d_class 1. */
int xAlfClassifyGpu (x266hip_ctx *ctx, const x266_ref_block_t *d_dec, int width, int height, uint8_t *d_class, void *stream);
/* Alignment in bytes: d_org 16, d_dec 16, d_class 1, d_stats 4. */
int xAlfStatsGpu    (x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height,
                     const uint8_t *d_class, int32_t *d_stats, void *stream);
/* Alignment in bytes: d_stats 4, d_mask 1, d_total 8. */
int xAlfSumStatsGpu (x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, const uint8_t *d_mask, int64_t *d_total,
                     void *stream);
/* Alignment in bytes: d_stats 4, d_luma 4, d_chroma 4, d_ctrl 1. */
int xAlfDecideGpu   (x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, const x266_alf_luma_t *d_luma, int n_luma,
                     const x266_alf_chroma_t *d_chroma, int n_chroma, int lambda_q4, uint8_t *d_ctrl, void *stream);
/* Alignment in bytes: d_in 16, d_class 1, d_luma 4, d_chroma 4, d_ctrl 1, d_out 16. */
int xAlfApplyGpu    (x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const uint8_t *d_class,
                     const x266_alf_luma_t *d_luma, int n_luma, const x266_alf_chroma_t *d_chroma, int n_chroma,
                     const uint8_t *d_ctrl, x266_ref_block_t *d_out, void *stream);
/* Sum of absolute differences of n_blocks pairs of edge x edge 8-bit blocks (edge in
 * {4, 8, 16, 32, 64}; each block edge*edge contiguous bytes, row-major; d_a and d_b 16-byte,
 * d_out 4-byte aligned): d_out[b] = sum |a - b|, exactly sad() of
 * riscv/programs/benchmarks/sad/sad.c:28-39 (whose 64 x 64 known answer 344807 the tests replay). */
/* Alignment in bytes: d_a 16, d_b 16, d_out 4. */
int xSadBatchDev(x266hip_ctx *ctx, int edge, const uint8_t *d_a, const uint8_t *d_b, uint32_t *d_out,
                 size_t n_blocks, void *stream);
/* 32x32 intra prediction.  Upstream has only a work-in-progress RTL sketch of this
 * stage (src/mkIntra32-wip.bsv; no C model, so parity is UNPINNED): the HEVC 35-mode predictor
 * (H.265 8.4.4.2.4-6, nTbS = 32) -- mode 0 planar, 1 DC, 2..34 angular -- on references used as
 * given.  x266_intra_ref_t mirrors IntraRef_t (:36-39): left[y] = p[-1][y], top[0] = the corner
 * sample, top[1+x] = p[x][-1]; padded to 144 bytes so that sets are 16-byte aligned.
 * Output block i (1024 bytes, row-major) = mode d_modes[i] on set d_ref_index[i] (NULL: set i).
 * d_refs and d_pred 16-byte, d_ref_index 4-byte aligned; d_modes is bytes at any address. */
typedef struct x266_intra_ref_t {
    uint8_t left[64];
    uint8_t top[65];
    uint8_t reserved[15];
} x266_intra_ref_t;
/* Alignment in bytes: d_refs 16, d_modes 1, d_ref_index 4, d_pred 16. */
int xIntra32PredictDev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_modes,
                       const uint32_t *d_ref_index, uint8_t *d_pred, size_t n, void *stream);
/* The encoder loop's form of intra coding, in ONE kernel: d_coef[i] = forward DCT32 (xDct32FwdBatchDev's transform,
 * src_tb/dct32.c:66-170,180-198) of the residual d_src[i] - prediction(mode d_modes[i] on set d_ref_index[i] (NULL: set i)).
 * The prediction never reaches memory: 1 KiB of source samples (row-major 32x32 uint8) + 144 bytes of references in, 2 KiB of
 * coefficients out per block.  Bit-identical to xIntra32PredictDev -> residual -> xDct32FwdBatchDev.  Modes above 34 are
 * undefined input, as for xIntra32PredictDev. */
/* Alignment in bytes: d_refs 16, d_modes 1, d_ref_index 4, d_src 16, d_coef 16. */
int xIntra32ResidualDct32Dev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index,
                             const uint8_t *d_src, int16_t *d_coef, size_t n, void *stream);
/* Intra mode decision (the sketch's "Decide" channel, IntraChannel_t :41-44): for block b with reference
 * set d_refs[b] and source samples d_src[b*1024 ..] (row-major 32x32, 16-byte aligned),
 * d_costs[b*35 + m] = sum over the sixteen 8x8 sub-blocks of satd8x8(src - prediction m)
 * (satd8x8 = src_tb/satd.c:31-118), m = 0..34; d_best_mode[b] (may be NULL) = the cheapest mode,
 * lowest index on ties.  The predictions are never written to memory.  d_costs 4-byte aligned, d_best_mode
 * bytes at any address. */
/* Alignment in bytes: d_refs 16, d_src 16, d_costs 4, d_best_mode 1. */
int xIntra32CostsDev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_src,
                     uint32_t *d_costs, uint8_t *d_best_mode, size_t n_blocks, void *stream);
/* Intra coding of tiled frames.  HEVC's 32x32 intra scheme at 8 bits as recalled, unverified offline; the arithmetic written here is the
 * contract.  width, height positive multiples of 64 (the caller pads); CTUs of 64x64 in raster order, n_ctu of them.
 *
 * The reference set of a 32x32 block is an x266_intra_ref_t: left[y] = p[-1][y], y = 0..63; top[0] = the corner sample;
 * top[1+x] = p[x][-1], x = 0..63; the 15 reserved bytes are written as 0.  It has five segments: BL = left[32..63], L = left[0..31],
 * C = top[0], T = top[1..32], TR = top[33..64].  A segment is available iff the 32x32 block that holds it lies inside the frame and
 * precedes the current block in coding order: CTUs in raster order, inside a CTU the luma quadrants q = 0, 1, 2, 3 (top-left,
 * top-right, bottom-left, bottom-right).  For luma block (bx, by) on the 32-sample grid, q = 2 (by & 1) + (bx & 1):
 *     L  = block (bx-1, by)    in the frame            T  = block (bx, by-1)    in the frame
 *     C  = block (bx-1, by-1)  in the frame            TR = block (bx+1, by-1)  in the frame and q != 3
 *     BL = block (bx-1, by+1)  in the frame and q == 0
 * For the 32x32 U or V block of CTU (cx, cy), on its own plane, in a frame ctus_x CTUs wide:
 *     L: cx > 0     T: cy > 0     C: cx > 0 and cy > 0     TR: cy > 0 and cx + 1 < ctus_x     BL: never
 * Substitution (H.265 8.4.4.2.2): order the 129 samples left[63], ..., left[0], top[0], top[1], ..., top[64].  If none is available,
 * every sample is 128.  Otherwise every sample in front of the first available one takes that one's value, and every later
 * unavailable sample takes the value of its predecessor in this order.  No reference smoothing filter and no DC / horizontal /
 * vertical edge filter is applied (xIntra32PredictDev has none, and HEVC has no edge filter at 32).
 *
 * xIntra32RefsFromTilesGpu -- the open-loop gather: the sets of a frame's OWN samples under exactly this rule.  component 0 (luma,
 * m_Y): 4 n_ctu sets, d_refs[4 ctu + q]; component 1 (U) or 2 (V) (the even / odd bytes of m_C): n_ctu sets, d_refs[ctu].  It
 * connects xIntra32CostsDev / PredictDev / ResidualDct32Dev to tiled frames; on the source frame it gives the open-loop mode
 * decision of a whole frame in one launch.  m_I is never read.  d_frame and d_refs are 16-byte aligned.  X266HIP_EINVAL for a NULL
 * or misaligned pointer, a bad size, a component outside 0..2, a span that does not fit in the address space, or d_refs
 * overlapping d_frame.
 *
 * xIntra32CodeFrameGpu -- the closed loop, in which a block's references are the reconstructed samples of its neighbours.  Regions
 * are 6 ctu + q as for xDct32CodeCtuTilesGpu: Y0 Y1 Y2 Y3 U V.  For every CTU in coding order and every luma quadrant q:
 *   1. the set is gathered from m_Y of d_recon by the rule above;
 *   2. the mode: d_mode_in == NULL: the mode of least xIntra32CostsDev cost -- the sum over the sixteen 8x8 sub-blocks of
 *      satd8x8(cur - prediction m), m = 0..34, the lowest index on ties; otherwise d_mode_in[6 ctu + q] (modes above 34 are
 *      undefined input, as for xIntra32PredictDev);
 *   3. pred = the xIntra32PredictDev prediction of that mode on that set;
 *   4. level = Q(DCT32(cur - pred)) with n = 5, the region's qp = min(d_qp[6 ctu + q], 51), or the scalar qp when d_qp == NULL,
 *      and `rounding`, exactly as xQuantRegionsGpu;
 *   5. recon = clip8(pred + IDCT32(Q^-1(level))) into m_Y of d_recon.
 * Then U and V of the CTU: one set per plane from m_C of d_recon; both planes share ONE mode out of the candidate list
 * (0, 26, 10, 1, the mode chosen for quadrant 0), in that order: cost(m) = cost_U(m) + cost_V(m), each the same 16-sub-block SATD
 * sum on its plane; least cost wins, the first in the list on ties (a duplicate candidate is harmless).  With d_mode_in,
 * d_mode_in[6 ctu + 4] serves both planes and entry 5 is ignored.  U is coded with the qp of region 4 and V with that of region 5,
 * steps 3 to 5 as for luma, into m_C of d_recon.
 * Outputs: d_level[ctu * 6144 + q * 1024 ..] and d_nnz[6 ctu + q] (d_nnz may be NULL), laid out as xDct32CodeCtuTilesGpu writes
 * them; d_mode[6 ctu + q] = the mode used, entries 4 and 5 both the chroma mode; m_Y and m_C of d_recon.  m_I of d_recon is never
 * read or written and m_I of d_cur is never read.  d_mode == d_mode_in is allowed; any other overlap of an output with any buffer
 * of the call returns X266HIP_EINVAL, d_recon == d_cur included.
 * Schedule: the dependence is serial by nature, so the call is a sequence of launches on the caller's stream, one per step, and
 * stream order is its only synchronisation (no workgroup waits for another): region (cx, cy, q) runs at step 4 cx + 6 cy + q and a
 * CTU's chroma at its q = 3 step, 4 ctus_x + 6 ctus_y - 6 steps in all; the result does not depend on the schedule.
 * d_cur, d_recon and d_level are 16-byte aligned, d_nnz 4-byte; d_qp, d_mode_in and d_mode are bytes at any address.
 * X266HIP_EINVAL for a NULL (d_cur, d_level, d_mode, d_recon) or misaligned pointer, a bad size, a scalar qp outside 0..51 when
 * d_qp == NULL, rounding outside 0..511, or a span that does not fit in the address space.
 * Both calls allocate nothing and can be captured into a graph; a refused call launches nothing and names itself in xHipLastError. */
/* Alignment in bytes: d_frame 16, d_refs 16. */
int xIntra32RefsFromTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_frame, int width, int height, int component,
                             x266_intra_ref_t *d_refs, void *stream);
/* Alignment in bytes: d_cur 16, d_qp 1, d_mode_in 1, d_level 16, d_nnz 4, d_mode 1, d_recon 16. */
int xIntra32CodeFrameGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, int width, int height, const uint8_t *d_qp, int qp,
                         int rounding, const uint8_t *d_mode_in, int16_t *d_level, uint32_t *d_nnz, uint8_t *d_mode,
                         x266_ref_block_t *d_recon, void *stream);

/* ---- mixed inter / intra coding of a frame: intra 32x32 regions in P- and B-frames ----
 * xDct32CodeMixedFrameGpu codes a frame whose regions are predicted either from another frame (d_pred, as any xMotionComp* call
 * writes m_Y and m_C) or from the frame itself (the 32x32 intra predictor on the reconstructed neighbours), region by region: where
 * motion compensation fails -- uncovered background, a new object, a partial scene change -- the region falls back to intra and
 * the frame stays on the device.  Regions are 6 ctu + q in the order Y0 Y1 Y2 Y3 U V, CTUs in raster order, the luma quadrants
 * q = 0..3 inside each CTU; the coding order of the frame is the one xIntra32CodeFrameGpu defines.
 *
 * For every luma quadrant, r = 6 ctu + q:
 *   1. k = d_kind_in ? min(d_kind_in[r], 2) : 2.  0 = inter, 1 = intra, 2 = the call decides.
 *   2. If k >= 1 the reference set is gathered from m_Y of d_recon by the availability and substitution rule of
 *      xIntra32CodeFrameGpu, unchanged: a neighbour of either kind counts as available once it precedes the block.
 *   3. Costs, both the sum over the sixteen 8x8 sub-blocks of satd8x8(cur - prediction): inter_cost with the prediction of
 *      d_pred; intra_cost the least cost over the candidate modes, the lowest index on ties.  The candidates are all 35 modes
 *      when d_mode_in == NULL, otherwise the one mode d_mode_in[r] (modes above 34 are undefined input).
 *   4. Decision.  k == 2: the region is intra iff intra_cost + intra_penalty < inter_cost; a tie is inter.  k == 0 or 1: the kind
 *      is given.  intra_penalty is what intra has to beat inter by, the call's only rate term: with inter_cost 6087 and
 *      intra_cost 4699 the region is intra at penalty 0 and at 1387, and inter at 1388 (the tie) and at 4096.
 *   5. Coding.  Inter: level = Q(DCT32(cur - pred)), recon = clip8(pred + IDCT32(Q^-1(level))), exactly as xDct32CodeCtuTilesGpu.
 *      Intra: steps 3 to 5 of xIntra32CodeFrameGpu with the chosen mode.
 * Then U and V of the CTU, which share ONE kind and ONE mode: k from entry 4 (entry 5 is ignored); one set per plane from m_C of
 * d_recon; with d_mode_in == NULL the intra candidates are (0, 26, 10, 1), followed by quadrant 0's mode only if quadrant 0 ended
 * intra, otherwise the one mode d_mode_in[6 ctu + 4]; cost(m) = cost_U(m) + cost_V(m), the first in the list on ties; inter_cost =
 * cost_U + cost_V against d_pred; the same comparison with the same intra_penalty decides.  U is coded with the qp of region 4 and V
 * with that of region 5.
 * Outputs.  d_level and d_nnz as the two existing coding calls write them.  d_kind[r] = the kind the region ended with, 0 or 1;
 * d_mode[r] = the mode used, 255 for an inter region; entries 4 and 5 both hold the chroma kind and mode.  d_cost[2 r] = inter_cost,
 * written for k == 2; d_cost[2 r + 1] = intra_cost, written for k == 2, and for k == 1 when d_mode_in == NULL; every other entry is
 * 0xFFFFFFFF; entry 5 repeats entry 4.  m_Y and m_C of d_recon; m_I of d_recon is never read or written.
 * Overlap.  d_recon == d_pred is allowed and is the form an encoder uses: a region reads its own prediction before it writes its own
 * reconstruction and reads only earlier regions of d_recon.  d_kind == d_kind_in and d_mode == d_mode_in are allowed.  Any other
 * overlap of an output with any buffer of the call returns X266HIP_EINVAL, d_recon == d_cur included.
 *
 * What follows from it:
 *   (a) with every kind 0, d_level, d_nnz and d_recon are bit for bit those of xDct32CodeCtuTilesGpu on the same arguments;
 *   (b) with every kind 1, d_level, d_nnz, d_mode and d_recon are bit for bit those of xIntra32CodeFrameGpu, and d_pred is never read;
 *   (c) a region's result depends only on regions before it in coding order, so it does not depend on the schedule;
 *   (d) entries 0..3 of every CTU of d_kind are exactly what x266_deblock_t.d_intra reads: d_kind is a valid d_intra.
 * Schedule (not part of the contract): one launch codes every region whose d_kind_in byte is 0 -- they depend on nothing -- and the
 * wavefront of xIntra32CodeFrameGpu follows, one launch per step on the caller's stream, in which a workgroup whose region was given
 * as inter returns after reading that byte.  Stream order is the only synchronisation.  A caller that screens the regions (with
 * xLaFrameCostGpu's decision, say) and marks only the doubtful ones 2 pays the steps in launch overhead plus those regions.
 * One host struct, read during the call; the pointers in it are device pointers (alignments: the field comments).  The call
 * allocates nothing and can be captured into a graph.  X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a
 * NULL p, a NULL or misaligned required buffer, a side that is not a positive multiple of 64, a scalar qp outside 0..51 when
 * d_qp == NULL, rounding outside 0..511, intra_penalty outside 0 .. 1 << 24, a span that does not fit in the address space, and
 * an overlap other than the three above.  With n = 6 n_ctu the extents are width * height * 2 (the frames), n bytes (d_qp, the
 * kinds, the modes), 2048 n (d_level), 4 n (d_nnz) and 8 n (d_cost). */
typedef struct x266_mixed_t {
    const x266_ref_block_t *d_cur;         /* the source frame, [(width / 16) * (height / 16)], 16-byte aligned                 */
    const x266_ref_block_t *d_pred;        /* the inter prediction, the same size, 16-byte aligned; m_Y and m_C are read        */
    const uint8_t *d_qp;                   /* [6 n_ctu] or NULL, 1-byte aligned; NULL: the scalar qp                            */
    const uint8_t *d_kind_in;              /* [6 n_ctu] or NULL, 1-byte aligned; 0 inter, 1 intra, 2 and above decide           */
    const uint8_t *d_mode_in;              /* [6 n_ctu] or NULL, 1-byte aligned; NULL: the call chooses the intra mode          */
    int16_t *d_level;                      /* [6 n_ctu * 1024], 16-byte aligned; output                                         */
    uint32_t *d_nnz;                       /* [6 n_ctu] or NULL, 4-byte aligned; output                                         */
    uint8_t *d_kind;                       /* [6 n_ctu], 1-byte aligned; output, may be d_kind_in                               */
    uint8_t *d_mode;                       /* [6 n_ctu], 1-byte aligned; output, may be d_mode_in                               */
    uint32_t *d_cost;                      /* [2 * 6 n_ctu] or NULL, 4-byte aligned; output                                     */
    x266_ref_block_t *d_recon;             /* the reconstruction, the frames' size, 16-byte aligned; output, may be d_pred      */
    int width, height;                     /* positive multiples of 64                                                          */
    int qp, rounding;                      /* qp 0..51, checked only when d_qp == NULL; rounding 0..511                         */
    int intra_penalty;                     /* 0 .. 1 << 24                                                                      */
} x266_mixed_t;
int xDct32CodeMixedFrameGpu(x266hip_ctx *ctx, const x266_mixed_t *p, void *stream);

/* ---- the compact level stream: what leaves the device for the host's entropy coder, and what a host decoder hands back ----
 * xDct32CodeCtuTilesGpu, xIntra32CodeFrameGpu and xQuantRegionsGpu(0) emit levels dense, 2 KiB per region, nearly all zeros at
 * any useful qp.  xLevelsPackGpu turns them into coded-group flags, significance maps and the non-zero levels in the order a
 * coefficient coder walks them; xLevelsUnpackGpu is the exact inverse and the entry of a decoder into xQuantRegionsGpu(1).
 *
 * Units.  A region is 1024 int16 levels (the unit of xQuantRegionsGpu and of the 12 KiB-per-CTU layouts).  Region r has the block
 * size N = 4 << (d_class[r] & 3) -- the class byte read exactly as xQuantRegionsGpu and xTransformTilesDev read it; d_class ==
 * NULL: N = 32 -- and is (32 / N)^2 blocks, block-major in raster order, each block row-major N x N: level (blk, v, u) is
 * d_level[r * 1024 + blk * N * N + v * N + u], u the horizontal and v the vertical frequency.
 * Diagonal scan of an M x M grid: the positions (x, y) ordered by x + y ascending, then by x ascending (the up-right diagonal of
 * HEVC and VVC).  For M = 4, scan index -> y * 4 + x is 0 4 1 8 5 2 12 9 6 3 13 10 7 14 11 15.
 * Coefficient groups.  A block is (N / 4)^2 CGs of 4x4; CG (cgx, cgy) covers u = 4 cgx .. 4 cgx + 3, v = 4 cgy .. 4 cgy + 3.  The CGs
 * of a block are ordered by the diagonal scan of the (N / 4) x (N / 4) grid, the 16 levels of a CG by the 4x4 scan.  A region always
 * has 64 CGs; CG bit g = blk * (N / 4)^2 + s, s the CG's scan position in its block.
 *
 * Per region one 32-byte record (below).  The payload of region r is d_stream[offset .. offset + n_words), in 16-bit words:
 * first one 16-bit significance map per coded CG, in ascending bit order of cg_mask -- bit i of a map is set when scan position i
 * of that CG is non-zero --, then the non-zero levels of those CGs as int16, CG by CG in the same order, in ascending scan position
 * inside each CG.  (Maps first: an unpacking lane finds its map from cg_mask alone and its levels from a prefix sum of popcounts.)
 * At most 64 + 1024 = 1088 words per region.  offset[r] is the exclusive prefix sum of n_words over regions 0 .. r - 1, in 64 bits:
 * a region's place depends on the data alone, and the same input gives the same bytes on every run.
 *
 * Both calls take one host struct, read during the call; the pointers in it are device pointers (alignments: the field comments).
 *
 * xLevelsPackGpu writes every record.  d_total[0] = the total number of words, d_total[1] = the number of leading regions whose
 * payload lies completely inside cap_words (n_regions exactly when the stream fits).  The payload of region r is written if and only
 * if offset + n_words <= cap_words; no word at or beyond cap_words is ever written.  cap_words == 0 with d_stream == NULL is the
 * count-only call: records and totals to size a buffer with.  With d_nnz != NULL a region with d_nnz[r] == 0 counts as all zero and
 * its levels are not read (the coding calls produce that array).  n_regions == 0 writes d_total = {0, 0} and nothing else.
 * Three launches on the caller's stream: count and records, the offsets (one workgroup, xLevelsScanChunk() regions per step), write.
 *
 * xLevelsUnpackGpu writes all 1024 levels of every region, absent ones as zeros, and with d_nnz != NULL the region's non-zero count
 * (what xDeblockGpu reads).  It trusts nothing in a record except cg_mask and offset: it reads the maps from the stream and derives
 * every count from them.  With end = offset + popcount(cg_mask) + the sum of popcount(map), a region with end > cap_words, or whose
 * maps alone already pass cap_words, is written as all zero with d_nnz[r] = 0.  A map of 0 under a set mask bit is legal and
 * contributes no level.  Nothing outside [0, cap_words) of the stream is ever read: the stream comes from a host decoder.
 * d_total is ignored; d_stream may be NULL when cap_words == 0.
 *
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned required buffer, a span
 * that does not fit in the address space, an output overlapping any other buffer.  The extents are n_regions * 2048 (d_level),
 * n_regions (d_class), n_regions * 4 (d_nnz), n_regions * 32 (d_region), cap_words * 2 (d_stream) and 16 bytes (d_total).  With
 * n_regions == 0 only d_total of the pack call is looked at.  Neither call allocates; both can be captured into a graph. */
typedef struct x266_level_region_t {
    uint64_t cg_mask;   /* bit g set: CG g has a non-zero level                      */
    uint64_t offset;    /* start of the region's payload in d_stream, in 16-bit words */
    uint32_t n_words;   /* popcount(cg_mask) + n_nz                                   */
    uint32_t n_nz;      /* non-zero levels of the region (what d_nnz holds)           */
    uint32_t sum_abs;   /* sum of |level|: the rate proxy a rate control wants        */
    uint32_t max_abs;   /* 0..32768: tells the host which binarisation range it needs */
} x266_level_region_t;
typedef struct x266_levels_t {
    int16_t  *d_level;                 /* [n_regions * 1024], 16-byte aligned; pack reads, unpack writes            */
    const uint8_t *d_class;            /* [n_regions] or NULL (every region 32x32), any alignment                   */
    uint32_t *d_nnz;                   /* [n_regions] or NULL, 4-byte aligned; pack reads, unpack writes (above)    */
    x266_level_region_t *d_region;     /* [n_regions], 8-byte aligned; pack writes, unpack reads                    */
    uint16_t *d_stream;                /* [cap_words], 16-byte aligned; pack writes, unpack reads                   */
    uint64_t *d_total;                 /* [2], 8-byte aligned; pack writes, unpack ignores (may be NULL there)      */
    size_t    n_regions;
    uint64_t  cap_words;
} x266_levels_t;
int xLevelsPackGpu  (x266hip_ctx *ctx, const x266_levels_t *p, void *stream);
int xLevelsUnpackGpu(x266hip_ctx *ctx, const x266_levels_t *p, void *stream);

/* ---- rate-distortion optimised quantisation (RDOQ) and a rate estimate of a region's levels ----
 * xQuantRegionsGpu(0) rounds every coefficient on its own.  xRdoQuantRegionsGpu weighs each level's distortion against what the level
 * costs to code, drops coefficient groups and trailing levels that do not pay, and reports distortion and estimated bits per region;
 * xLevelsBitsGpu gives the same estimate for levels from any producer.  No upstream counterpart: the RDOQ of HM, VTM and x265 in
 * outline, as recalled, with a static rate model; the arithmetic here is the contract.  All values are mathematical integers, every
 * one fits in int64.
 *
 * Region and block.  Region, class byte and block layout exactly as xQuantRegionsGpu and xLevelsPackGpu read them: N = 4 << (class &
 * 3), n = log2 N, d_class == NULL: N = 32; qp = min(d_qp[r], 51), or the scalar qp when d_qp == NULL.  The scan of a block is
 * xLevelsPackGpu's (xLevelScan): index i is a position in that order, s = i / 16 its CG, (u, v) its frequency.
 *
 * Rate, in 1/16 bit, a static model: no adaptive contexts, so regions and CGs are independent.
 *     position class: 0 at u = v = 0; 1 elsewhere in CG 0 (u < 4 and v < 4); 2 otherwise
 *     sig[class][0/1] = {24,10}, {12,22}, {6,36}     gt1[0/1] = {10,24}     gt2[0/1] = {11,22}     cgf[0/1] = {9,26}     a sign: 16
 *     rem(r), r >= 0:  r + 1 for r < 3, otherwise 3 + 2 ilog2(r - 2) + 1
 *     R(l, class), l a level magnitude:
 *         l = 0: sig[class][0]                                  l = 1: sig[class][1] + 16 + gt1[0]
 *         l = 2: sig[class][1] + 16 + gt1[1] + gt2[0]           l >= 3: sig[class][1] + 16 + gt1[1] + gt2[1] + 16 rem(l - 3)
 *     Rlast(u, v) = 16 (pos(u) + pos(v)),  pos(t) = min(g + 1, 2n - 1) + (g >= 4 ? (g >> 1) - 1 : 0),
 *         g = t for t < 4, otherwise g = 2 ilog2(t) + ((t >> (ilog2(t) - 1)) & 1)
 * Distortion.  a = |c|, x = a * f[qp % 6], f and qbits the quantiser's (above).  For a level magnitude l:
 *     err = |x - (l << qbits)|,   e = (err + (1 << (qbits - 9))) >> (qbits - 8)   (1/256 of a level),   D(l) = e * e
 *     J(l) = D(l) + lambda * R(l, class),   lambda an integer 0..8192, in 1/4096 of a squared level per bit.
 * The conventional 0.57 * 2^((qp - 12) / 3) in sample units comes to about 368 in these units at every qp; nobody has measured
 * which lambda serves this rate model best.
 *
 * Step 1, per coefficient.  h = (x + (1 << (qbits - 1))) >> qbits.  Candidates: h; h - 1 if h >= 1; 0 if h <= 2.  q[i] is the
 * candidate of least J; on a tie the smallest level wins.
 * Step 2, per CG with s >= 1 that has a non-zero q.  Jc = sum J(q[i]) + lambda * cgf[1], Jz = sum D(0) + lambda * cgf[0] over its 16
 * positions; the CG becomes all zero iff Jz < Jc.  CG 0 of a block is never touched here.
 * Step 3, per block that still has a non-zero level.  C(s), the cost of CG s: sum J(q[i]) for s = 0; sum J(q[i]) + lambda * cgf[1]
 * for a later CG with a non-zero level; sum D(0) + lambda * cgf[0] for a later CG with none.  For every p with q[p] != 0, s_p its CG,
 *     Total(p) = sum over s < s_p of C(s)  +  sum over i in CG s_p with i < p of J(q[i])
 *              + D(q[p]) + lambda * (R(q[p], class_p) - sig[class_p][1])  +  sum over all i > p of D(0)  +  lambda * Rlast(u_p, v_p)
 *     Total(none) = sum over all i of D(0).
 * The block's last position is the p of least Total; on a tie the larger p wins, and any p wins over none.  Every level after the
 * chosen p becomes 0; if none is chosen, every level becomes 0.  Signs are the coefficients'.
 *
 * Per region (x266_rdoq_region_t): dist = sum of D(final level) over its 1024 positions.  bits = the sum, over its blocks with a
 * non-zero level, p the block's last non-zero position, of Rlast(p) + cgf[coded] for every CG with 0 < s < s_p + R(level) for every
 * i <= p inside CG 0, CG s_p and the non-empty CGs between - sig[class_p][1].  bits is a function of the levels alone (not of
 * lambda); n_nz is the number of non-zero levels.
 *
 * xRdoQuantRegionsGpu turns d_coef into d_level by steps 1 to 3 (in place, d_level == d_coef, is allowed) and writes d_nnz and d_stat
 * when given.  Its levels feed xQuantRegionsGpu(1), xLevelsPackGpu and the deblocking calls exactly as the plain quantiser's do.
 * xLevelsBitsGpu reads d_level and writes d_stat with bits and n_nz as above and dist = 0; with d_nnz != NULL a region with d_nnz[r]
 * == 0 is not read and reports zeros.  It ignores d_coef, d_qp, qp and lambda.
 * One launch each on the caller's stream; neither call allocates, both can be captured into a graph, and the same input gives the
 * same bytes on every run.  n_regions == 0 returns 0 and launches nothing.  X266HIP_EINVAL, with nothing launched and the call
 * named in xHipLastError: a NULL p, a NULL or misaligned required buffer, qp (without d_qp) or lambda out of range
 * (xRdoQuantRegionsGpu), a span that does not fit in the address space, any overlap of an output with another buffer other than
 * d_level == d_coef.  The extents are n_regions * 2048 (d_coef, d_level), n_regions (d_class, d_qp), n_regions * 4 (d_nnz) and
 * n_regions * 16 (d_stat). */
typedef struct x266_rdoq_region_t {
    uint64_t dist;      /* sum of D(final level), 1/65536 of a squared level; 0 from xLevelsBitsGpu */
    uint32_t bits;      /* estimated rate of the region's levels, 1/16 bit                         */
    uint32_t n_nz;      /* non-zero levels of the region (what d_nnz holds)                        */
} x266_rdoq_region_t;
typedef struct x266_rdoq_t {
    const int16_t *d_coef;             /* [n_regions * 1024], 16-byte aligned; NULL for xLevelsBitsGpu                       */
    int16_t *d_level;                  /* [n_regions * 1024], 16-byte aligned; rdoq writes (may be d_coef), bits reads       */
    const uint8_t *d_class;            /* [n_regions] or NULL (every region 32x32), any alignment                            */
    const uint8_t *d_qp;               /* [n_regions] or NULL, any alignment                                                 */
    uint32_t *d_nnz;                   /* [n_regions] or NULL, 4-byte aligned; rdoq writes, bits reads (0 = skip the region) */
    x266_rdoq_region_t *d_stat;        /* [n_regions], 8-byte aligned; rdoq: may be NULL; bits: required                     */
    size_t n_regions;
    int qp, lambda;                    /* qp 0..51 checked only when d_qp == NULL; lambda 0..8192                            */
} x266_rdoq_t;
int xRdoQuantRegionsGpu(x266hip_ctx *ctx, const x266_rdoq_t *p, void *stream);
int xLevelsBitsGpu     (x266hip_ctx *ctx, const x266_rdoq_t *p, void *stream);

/* ---- transform decision: each region's class byte by rate-distortion cost ----
 * The source of d_class.  xTransformCtuFromTilesDev / ToTilesDev, xQuantRegionsGpu, xRdoQuantRegionsGpu, xLevelsBitsGpu and
 * xLevelsPackGpu / UnpackGpu read a class byte X266_TILE_CLASS(type, size) per 32x32 region; xTransformDecideCtuTilesGpu chooses it, per
 * region, among the caller's candidates and writes the winner's levels with it.  dist and bits of x266_rdoq_region_t are in
 * quantiser-step units for every class (the transforms' shifts and qbits = 14 + qp/6 + (7 - n) cancel N), so they compare across sizes.
 * No upstream counterpart; the composition of the calls above is the contract.  All values are mathematical integers.
 *
 * Frame, CTUs and regions exactly as xTransformCtuFromTilesDev: width and height positive multiples of 16, n_ctu = ceil(width / 64) *
 * ceil(height / 64), n = 6 n_ctu regions in the order 6 ctu + q (q: Y0 Y1 Y2 Y3 U V), samples outside the frame are residual 0 and
 * every region slot is written.  qp = min(d_qp[r], 51), or the scalar qp when d_qp == NULL; lambda as in x266_rdoq_t.
 * Candidates are uint16 masks over class byte values, bit k = class byte k; the valid bits are X266_TDECIDE_CLASSES: the 13 distinct
 * classes, size 32 only as class 3 (DCT-II; the set has one 32-point matrix).  The effective mask of region r is d_cand[r] &
 * X266_TDECIDE_CLASSES when d_cand != NULL and that is non-zero, otherwise cand_luma for q = 0..3 and cand_chroma for q = 4, 5.  The
 * call applies no divisibility rule of its own, as the transform calls check no class byte: an encoder that wants no block to
 * straddle the frame edge in a cut region says so in d_cand.  class_bits[k] is the caller's cost of signalling class k, in 1/16 bit.
 *
 * For region r and every class k of its effective mask:
 *     C_k        = region r of xTransformCtuFromTilesDev run with every class byte equal to k
 *     (L_k, S_k) = what xRdoQuantRegionsGpu gives for C_k with class k, the region's qp and lambda
 *     J_k        = S_k.dist + lambda * (S_k.bits + class_bits[k])        (dist < 2^54, lambda * (...) < 2^34: J_k fits uint64)
 * The winner is the k of least J_k; on a tie the smallest class byte wins.  d_class[r] = the winner, a value in 0..14; d_level gets
 * the winner's L_k, block-major for its class; d_nnz and d_stat get the winner's S_k; d_cost[16 r + k] = J_k for the candidates and
 * all ones for every other k.  A region wholly outside the frame follows the same rule: its residual is 0, every J_k = lambda *
 * class_bits[k].  The outputs feed xQuantRegionsGpu(1, d_class), xTransformCtuToTilesDev(d_class), the deblocking calls (d_nnz) and
 * xLevelsPackGpu(d_class) unchanged.
 *
 * One launch on the caller's stream, one region per wave, no atomics and no ordering between waves: the same input gives the same
 * bytes on every run.  The call allocates nothing and can be captured into a graph.  It uses the context's installed transform
 * matrices and returns X266HIP_EDEVICE when the tables are invalid.  X266HIP_EINVAL, with nothing launched and the call named in
 * xHipLastError: a NULL p, a NULL or misaligned required buffer, a width or height that is not a positive multiple of 16, qp (without
 * d_qp) or lambda out of range, a mask with a bit outside X266_TDECIDE_CLASSES or with no bit set, a span that does not fit in the
 * address space, any overlap of an output with any other buffer of the call (d_cur == d_pred, two inputs, is allowed).  The extents
 * are width * height * 2 (d_cur, d_pred), n (d_qp, d_class), n * 2 (d_cand), n * 2048 (d_level), n * 4 (d_nnz), n * 16 (d_stat) and
 * n * 128 (d_cost). */
#define X266_TDECIDE_CLASSES 0x777F
typedef struct x266_tdecide_t {
    const x266_ref_block_t *d_cur;     /* tiled frame, width * height * 2 bytes, 16-byte aligned                              */
    const x266_ref_block_t *d_pred;    /* tiled frame, width * height * 2 bytes, 16-byte aligned; may be d_cur                */
    const uint8_t *d_qp;               /* [n] or NULL, any alignment                                                          */
    const uint16_t *d_cand;            /* [n] or NULL, 2-byte aligned; the per-region candidate masks                         */
    uint8_t *d_class;                  /* [n], any alignment; the winners                                                     */
    int16_t *d_level;                  /* [n * 1024], 16-byte aligned; the winners' levels                                    */
    uint32_t *d_nnz;                   /* [n] or NULL, 4-byte aligned                                                         */
    x266_rdoq_region_t *d_stat;        /* [n] or NULL, 8-byte aligned                                                         */
    uint64_t *d_cost;                  /* [n * 16] or NULL, 8-byte aligned; J_k, all ones where k is no candidate             */
    int width, height;                 /* positive multiples of 16                                                            */
    int qp, lambda;                    /* qp 0..51 checked only when d_qp == NULL; lambda 0..8192                             */
    uint16_t cand_luma, cand_chroma;   /* masks within X266_TDECIDE_CLASSES, at least one bit each                            */
    uint16_t class_bits[16];           /* side-information cost of class k, 1/16 bit                                          */
} x266_tdecide_t;
int xTransformDecideCtuTilesGpu(x266hip_ctx *ctx, const x266_tdecide_t *p, void *stream);

/* ---- source analysis: tile activity, the adaptive qp map and fade weights, in front of the searches and the coding calls ----
 * One pass over the tiled source frame gives per-tile sums and sums of squares; from them come the qp byte per region that
 * xQuantRegionsGpu, xDct32CodeCtuTilesGpu, xIntra32CodeFrameGpu and x266_deblock_t take as d_qp, and the x266_wp_t of the
 * bi-directional calls.  No upstream counterpart: x264's adaptive quantisation and weight analysis, as recalled; the arithmetic here
 * is the contract.  Frame sides are positive multiples of 16; tiles are 16x16 in raster order, width / 16 per row.
 *
 * Per tile (m_Y 256 bytes; m_C even bytes U, odd bytes V, 64 each; m_I is never read), all uint32 and all products unsigned
 * (sum_y * sum_y reaches 65280^2, which fits uint32 and not int32):
 *   sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v                  the sums of the samples and of their squares
 *   energy  = (ssq_y - ((sum_y * sum_y) >> 8)) + (ssq_u - ((sum_u * sum_u) >> 6)) + (ssq_v - ((sum_v * sum_v) >> 6))   <= 6242400
 *   log2_q8 = L(energy)
 * L(e) = floor(256 log2(max(e, 1))), defined by: e = max(e, 1); k = 31 - clz(e); m = (uint64)e << (31 - k); f = 0; eight times
 * { m = (m * m) >> 31; f <<= 1; if (m >> 32) { f |= 1; m >>= 1; } }; L = (k << 8) | f.  L(0) = L(1) = 0, L(2) = 256, L(3) = 405,
 * L(1000) = 2551, L(6242400) = 5778.
 * Frame totals d_total[8]: the six sums over all tiles, then the sum of log2_q8, then the number of tiles.
 *
 * Per-tile offset in Q8: off = clamp((strength_q8 * (log2_q8 - ref_q8)) >> 8, -3072, 3072), the shift arithmetic.  mode 1 (fixed
 * reference): ref_q8 = 3693.  mode 2 (frame mean): ref_q8 = (d_total[6] + n_tiles / 2) / n_tiles, n_tiles the frame's.
 * Per-region qp d_qp[6 ctu + q]: CTUs are ceil(width / 64) x ceil(height / 64) in raster order; tile (tx, ty) lies in CTU
 * (tx >> 2, ty >> 2), quadrant q = ((ty >> 1) & 1) * 2 + ((tx >> 1) & 1).  For q = 0..3, S is the sum of off over the quadrant's
 * in-frame tiles and n their number; for q = 4, 5 both run over all in-frame tiles of the CTU.  delta = floor((2 S + 256 n) / (512 n))
 * (floor division: a mean offset of -128 gives 0, -129 gives -1, 128 gives 1), 0 when n = 0, and
 * qp = clamp(base qp + delta + (q >= 4 ? chroma_qp_offset : 0), 0, 51).  A region wholly outside the frame still gets its byte.
 *
 * Both device calls take one host struct, read during the call; the pointers in it are device pointers (alignments: the field
 * comments).  xAqStatsGpu reads d_src and writes every record of d_tile, then d_total: two launches on the caller's stream, the
 * second ONE workgroup that adds the records xAqTotalsChunk() at a time -- integer sums, no atomics, the same bytes on every run.
 * It looks at d_src, d_tile, d_total, width and height only.  xAqDecideGpu reads d_tile and d_total on the device (no host round
 * trip) and writes d_offset and d_qp, either of which may be NULL, not both; one launch.  Neither call allocates; both can be
 * captured into one graph.
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned required buffer, a
 * side that is not a positive multiple of 16, a span that does not fit in the address space, an output overlapping any other
 * buffer of the call, and in xAqDecideGpu a mode other than 1 or 2 or a scalar outside the ranges below.  The extents are
 * width * height * 2 (d_src), n_tiles * 32 (d_tile), 64 bytes (d_total), n_tiles * 2 (d_offset) and 6 n_ctu (d_qp). */
typedef struct x266_aq_tile_t {
    uint32_t sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v, energy, log2_q8;
} x266_aq_tile_t; /* 32 bytes */
typedef struct x266_aq_t {
    const x266_ref_block_t *d_src;     /* [n_tiles], 16-byte aligned; stats reads, decide ignores (may be NULL there)  */
    x266_aq_tile_t *d_tile;            /* [n_tiles], 16-byte aligned; stats writes, decide reads                       */
    int64_t  *d_total;                 /* [8], 8-byte aligned; stats writes, decide reads                              */
    int16_t  *d_offset;                /* [n_tiles] Q8 or NULL, 2-byte aligned; decide writes                          */
    uint8_t  *d_qp;                    /* [6 n_ctu] or NULL, any alignment; decide writes; one of the two is required  */
    int width, height;
    int mode;                          /* 1 or 2                                                                       */
    int strength_q8;                   /* 0..1024                                                                      */
    int qp;                            /* 0..51, the base qp                                                           */
    int chroma_qp_offset;              /* -12..12                                                                      */
} x266_aq_t;
int xAqStatsGpu (x266hip_ctx *ctx, const x266_aq_t *p, void *stream);
int xAqDecideGpu(x266hip_ctx *ctx, const x266_aq_t *p, void *stream);
/* Records the totals' workgroup of xAqStatsGpu takes per step (a test walks tile counts around it). */
int xAqTotalsChunk(void);
/* Fade weights from the totals of two frames of one size (host only; reads 8 int64 each, host memory).  list is 0 or 1: the call
 * writes wp->w[list][*] and wp->o[list][*] and reads wp->log2_denom, which the caller sets.  Per plane p of Y, U, V: N = the plane's
 * sample count (n_tiles * 256 for Y, n_tiles * 64 for U and V), var = ssq * N - sum^2, d = log2_denom[p ? 1 : 0],
 *   w = var_ref == 0 ? 1 << d : (isqrt((var_cur << (2 d + 2)) / var_ref) + 1) >> 1, then clamped to 1..127
 *   o = clamp(floor((2 (sum_cur 2^d - sum_ref w) + N 2^d) / (2 N 2^d)), -128, 127)
 * in exact integers (the variance products pass 2^63 at 8K).  X266HIP_EINVAL: list not 0 or 1, a NULL pointer, a log2_denom above
 * 7, cur[7] != ref[7], a tile count outside 1..2^24 or a negative total. */
int xWeightsFromTotals(const int64_t cur[8], const int64_t ref[8], int list, x266_wp_t *wp);

/* ---- lookahead: half-size frames, frame costs, scene cuts and the propagation tree ----
 * What a host needs to choose frame types and to weigh a block by what later frames predict from it, on data the device
 * already holds.  No upstream counterpart: x264's lookahead, as recalled; the arithmetic here is the contract.
 *
 * Geometry.  width, height: the full-resolution sides, positive multiples of 32.  The lowres frame is width / 2 x height / 2 (sides
 * W', H' multiples of 16), an ordinary tiled frame of n / 4 tiles that xSatd8x8SearchFromTilesDev searches as it is (called with
 * width / 2, height / 2).  n = (width / 16) * (height / 16) is the number of full-resolution tiles AND of lowres 8x8 blocks, both
 * in raster order, width / 16 per row: block b of the lowres frame (bx = b % (width / 16), by = b / (width / 16), at lowres
 * sample (8 bx, 8 by)) is tile b of the full-resolution frame.  n_ctu = ceil(width / 64) * ceil(height / 64).
 *
 * 1. xLaDownscaleGpu reads d_src and writes m_Y and m_C of every tile of d_low; m_I is neither read nor written.
 *    low(x, y) = (s(2x, 2y) + s(2x+1, 2y) + s(2x, 2y+1) + s(2x+1, 2y+1) + 2) >> 2 on the luma plane, and on the U plane (the even
 *    bytes of m_C) and the V plane (the odd bytes) separately: samples 1, 2, 3, 4 give 3; 0, 0, 0, 1 give 0; 0, 0, 1, 1 give 1;
 *    255, 255, 255, 254 give 255.  One launch.
 *
 * 2. xLaIntraCostsGpu reads m_Y of d_low and writes d_intra[b] and, when non-NULL, d_mode[b].  Neighbours of the block at
 *    (x0, y0) = (8 bx, 8 by), from the lowres frame's own samples p: top[x] = p(min(x0 + x, W' - 1), y0 - 1) and
 *    left[y] = p(x0 - 1, min(y0 + y, H' - 1)) for 0..8; TR = top[8], BL = left[8].  y0 == 0 and x0 == 0: all 18 are 128; only
 *    y0 == 0: every top[x] = left[0]; only x0 == 0: every left[y] = top[0].  Candidates, tried in this order, with the library's
 *    mode numbers:
 *       0 planar      ((7 - x) left[y] + (x + 1) TR + (7 - y) top[x] + (y + 1) BL + 8) >> 4
 *       1 DC          (sum top[0..7] + sum left[0..7] + 8) >> 4, no edge filter
 *      10 horizontal  left[y]
 *      26 vertical    top[x]
 *    With top = 10, 20, .., 90 and left = 100, 110, .., 180: planar(0, 0) = 65, planar(x = 3, y = 5) = 133, planar(7, 7) = 135,
 *    DC = 90.  cost(m) = satd8x8(cur - pred_m), the library's one SATD, (sum |H| + 2) >> 2 over the 8x8 Hadamard transform of the
 *    difference, at most 32640: a difference of 1 everywhere costs 16, one of +-255 in a checkerboard 4080, a block of 0 / 255
 *    in a checkerboard against 128 costs 2048.  The least cost wins, the first candidate of equal ones (a constant frame: cost 0,
 *    mode 0).  One launch.
 *
 * 3. xLaFrameCostGpu reads d_intra, d_mode (NULL: every mode counts as 0), d_inter0 and d_inter1 -- x266_me_result_t[n], what a
 *    search of two lowres frames writes; either or both may be NULL, with both NULL the call gives an I frame's cost -- and
 *    writes d_block[b], then d_total.  ci = d_intra[b] + intra_penalty (uint32; every cost is expected below 2^31).  best = list
 *    0 if present; list 1 replaces it only if its cost is strictly lower; intra replaces it only if ci is strictly lower, or if
 *    no list is present: ties go to list 0, then list 1, then intra.  Costs (l0, l1, d_intra) = (500, 500, 400) with penalty
 *    100: kind 1, cost 500; (500, 499, 400): kind 2, cost 499; (500, 500, 399): kind 0, cost 499.
 *    d_total (int64[8]): 0 sum of cost, 1 sum of intra, 2 / 3 / 4 the numbers of kind-0 / 1 / 2 blocks, 5 the sum of d_inter0's
 *    costs over ALL blocks (0 if NULL), 6 the same for d_inter1, 7 n.  Two launches on the caller's stream, the second ONE
 *    workgroup that adds xLaTotalsChunk() blocks per step: integer sums, no atomics, the same bytes on every run.
 *
 * 4. xSceneCutFromTotals (host only, plain integers; total: host memory, the result of a P decision against the previous frame).
 *    p = total[0], i = total[1], tmax = threshold_q8 << 8 (Q16), tmin = tmax >> 2, g = frames_since_key.  bias (Q16):
 *    4 g <= min_keyint: tmin >> 2; else g <= min_keyint: tmin * g / min_keyint; else tmin + (tmax - tmin) * (g - min_keyint) /
 *    (max_keyint - min_keyint), which is tmax when max_keyint == min_keyint.  Returns 1 when p * 65536 >= (65536 - bias) * i, else
 *    0.  threshold_q8 102, keyints 25 / 250: g = 5 gives bias 1632, g = 10 gives 2611, g = 100 gives 13056, and there p = 90000
 *    against i = 100000 is a cut, p = 80000 is none; keyints 25 / 25 at g = 30: 26112.  Returns -1 for a NULL total, threshold_q8
 *    outside 0..256, g < 0, min_keyint < 1, max_keyint < min_keyint, a negative total, total[7] outside 1..2^24, or p or i
 *    above 2^40 (every product fits int64).
 *
 * 5. xLaPropagateGpu, one step of the propagation tree: reads d_block and d_prop (uint64[n], what this frame has received so
 *    far; NULL counts as zeros) and ADDS into d_prop_ref0 and d_prop_ref1 (uint64[n], the accumulators of the list-0 and list-1
 *    reference frames), which the caller zeroes once, before the first frame that refers to them.  Either target may be NULL:
 *    blocks of that kind are skipped (both NULL: nothing is launched).  Per block: skipped when kind == 0 or intra == 0;
 *    q = min(d_prop[b], 2^32 - 1); inter = min(cost, intra); amount = ((intra + q) * (intra - inter)) / intra, floor, in
 *    unsigned 64 bits (intra is expected below 2^31); px = 8 bx + mvx, py = 8 by + mvy; X = floor(px / 8), dx = px - 8 X in
 *    0..7, Y and dy likewise.  Targets and weights w: (X, Y) (8 - dx)(8 - dy); (X + 1, Y) dx (8 - dy); (X, Y + 1) (8 - dx) dy;
 *    (X + 1, Y + 1) dx dy.  A target with w > 0 inside the block grid receives (amount * w + 32) >> 6; one outside is dropped and no
 *    byte is touched for it.  intra 1000, cost 600, d_prop 5000: amount 2400 (cost 1200: 0).  Block (1, 3) with mv (-11, 5): px = -3,
 *    X = -1, dx = 5, py = 29, Y = 3, dy = 5, weights 9, 15, 15, 25; (-1, 3) and (-1, 4) are dropped, (0, 3) receives 563 and (0, 4)
 *    938 (and 338 and 563 would have gone to the other two).  The adds are 64-bit integer atomic adds: they commute, so the result is
 *    the same bytes on every run whatever the schedule; one add is below 2^39 and n at most 2^24, so no sum overflows.  One launch.
 *
 * 6. xLaTreeQpGpu reads d_block (intra only), d_prop (NULL counts as zeros) and d_aq_offset (int16 Q8 per tile as xAqDecideGpu
 *    writes d_offset; NULL counts as zeros) and writes d_offset and / or d_qp: either may be NULL, not both.  Per tile t:
 *    P = min(d_prop[t], 2^32 - 1 - intra); gain = intra == 0 ? 0 : (strength_q8 * (L(intra + P) - L(intra))) >> 8 with L the
 *    source analysis' (never negative); off = clamp(aq - gain, -3072, 3072).  intra 1000 (L = 2551) with P = 3000 (L(4000) =
 *    3063): gain 1024 at strength 512, 2048 at 1024; intra 1 with d_prop 2^40 at 1024: 32764.  d_qp[6 ctu + q] comes from these
 *    offsets, the base qp and chroma_qp_offset by exactly the rule of xAqDecideGpu above (CTU and quadrant of a tile, delta, the
 *    clamp; a region wholly outside the frame still gets its byte).  One launch.
 *
 * All device calls take one host struct, read during the call; the pointers in it are device pointers (alignments: the field
 * comments).  Each call looks only at the fields named for it, width and height.  No call allocates; all can be captured into
 * one graph (the search between them needs xHipMeScratchReserve first).
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned required buffer, a
 * side that is not a positive multiple of 32, a span that does not fit in the address space, a scalar outside the range its
 * field comment states, xLaTreeQpGpu without an output, and an output -- or an accumulator being added into -- that overlaps
 * any other buffer of the call (d_prop_ref0 == d_prop_ref1 included).  The extents are width * height * 2 (d_src), width * height
 * / 2 (d_low), 4 n (d_intra), n (d_mode), 8 n (d_inter0, d_inter1, d_prop, d_prop_ref0, d_prop_ref1), 16 n (d_block), 64 bytes
 * (d_total), 2 n (d_aq_offset, d_offset) and 6 n_ctu (d_qp). */
typedef struct x266_la_block_t {
    uint32_t cost;        /* the minimum; with the penalty when intra        */
    uint32_t intra;       /* d_intra[b], without the penalty                 */
    int16_t  mvx, mvy;    /* the chosen list's vector, lowres pels; 0,0 intra */
    uint8_t  kind;        /* 0 intra, 1 list 0, 2 list 1                     */
    uint8_t  mode;        /* the intra mode (always, also for inter blocks)  */
    uint16_t reserved;    /* written as 0                                    */
} x266_la_block_t; /* 16 bytes */
typedef struct x266_la_t {
    const x266_ref_block_t *d_src;         /* [n], 16-byte aligned; downscale reads                                             */
    x266_ref_block_t *d_low;               /* [n / 4], 16-byte aligned; downscale writes, intra costs reads                     */
    uint32_t *d_intra;                     /* [n], 4-byte aligned; intra costs writes, frame cost reads                         */
    uint8_t  *d_mode;                      /* [n] or NULL, any alignment; intra costs writes, frame cost reads                  */
    const x266_me_result_t *d_inter0;      /* [n] or NULL, 8-byte aligned; frame cost reads                                     */
    const x266_me_result_t *d_inter1;      /* [n] or NULL, 8-byte aligned; frame cost reads                                     */
    x266_la_block_t *d_block;              /* [n], 16-byte aligned; frame cost writes, propagate and tree qp read               */
    int64_t  *d_total;                     /* [8], 8-byte aligned; frame cost writes                                            */
    const uint64_t *d_prop;                /* [n] or NULL, 8-byte aligned; propagate and tree qp read                           */
    uint64_t *d_prop_ref0;                 /* [n] or NULL, 8-byte aligned; propagate adds into                                  */
    uint64_t *d_prop_ref1;                 /* [n] or NULL, 8-byte aligned; propagate adds into                                  */
    const int16_t *d_aq_offset;            /* [n] Q8 or NULL, 2-byte aligned; tree qp reads                                     */
    int16_t  *d_offset;                    /* [n] Q8 or NULL, 2-byte aligned; tree qp writes                                    */
    uint8_t  *d_qp;                        /* [6 n_ctu] or NULL, any alignment; tree qp writes; one of the two is required      */
    int width, height;                     /* the full-resolution sides, positive multiples of 32                               */
    int intra_penalty;                     /* 0..65535; frame cost                                                              */
    int strength_q8;                       /* 0..1024; tree qp                                                                  */
    int qp;                                /* 0..51, the base qp; tree qp                                                       */
    int chroma_qp_offset;                  /* -12..12; tree qp                                                                  */
} x266_la_t;
int xLaDownscaleGpu (x266hip_ctx *ctx, const x266_la_t *p, void *stream);
int xLaIntraCostsGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream);
int xLaFrameCostGpu (x266hip_ctx *ctx, const x266_la_t *p, void *stream);
int xLaPropagateGpu (x266hip_ctx *ctx, const x266_la_t *p, void *stream);
int xLaTreeQpGpu    (x266hip_ctx *ctx, const x266_la_t *p, void *stream);
/* Blocks the totals' workgroup of xLaFrameCostGpu takes per step (a test walks block counts around it). */
int xLaTotalsChunk(void);
int xSceneCutFromTotals(const int64_t total[8], int threshold_q8, int frames_since_key, int min_keyint, int max_keyint);

/* ---- hierarchical motion search: a seeded SATD search around per-block starting vectors ----
 * The exhaustive searches score (2 range + 1)^2 candidates per block and stop at range 64.  This call scores a few small squares
 * around vectors the caller already has -- the winners of a search of the two half-size frames (xLaDownscaleGpu, then
 * xSatd8x8SearchFromTilesDev on them: a lowres range of 64 reaches 128 full-resolution samples), the previous frame's field, the other
 * list's field -- and charges every candidate the bits of its difference to the block's own seed, so that the field it hands to
 * xSatd8x8RefineQpelFromTilesGpu and the bi-directional calls is regularised.  No upstream counterpart; the arithmetic here is the
 * contract.  Whole samples, 8x8 luma blocks, the inter stage's edge rule (a reference sample outside the frame takes the nearest
 * in-frame one, any displacement is legal) and its one metric satd8x8 (src_tb/satd.c:31-118).
 *
 * Seed cell.  Block (bx, by) is the 8x8 luma block at (8 bx, 8 by), b = by * (width / 8) + bx.  Its seed cell is (sx, sy) =
 * (bx >> seed_scale, by >> seed_scale) of a grid of (width / 8 >> seed_scale) x (height / 8 >> seed_scale) cells, d_seed in raster
 * order.  seed_scale 0: one seed per block, in full-resolution samples (a previous field, the other list).  seed_scale 1: one seed per
 * 16x16 tile, in lowres samples -- exactly the d_best of a search of the two half-size frames.
 * Centre vectors.  S(sx, sy) = clamp(seed << seed_scale, -8183, 8183) per component, computed in 32 bits: a seed of -32768 gives
 * -8183 and 32767 gives 8183 at either scale, 4091 at scale 1 gives 8182, 4092 gives 8183.  Every candidate then lies inside
 * +-8191, which is what the quarter-sample refinement takes unclamped.
 * Ordered centre list of a block.  0 own: S(sx, sy), always.  Added only when its bit of `centres` is set: 1 (0, 0), bit 0;
 * 2 left: S(sx - 1, sy), bit 1; 3 top: S(sx, sy - 1), bit 2; 4 right: S(sx + 1, sy), bit 3; 5 bottom: S(sx, sy + 1), bit 4.  A
 * neighbour outside the seed grid is skipped, not substituted: with centres 31 the top-left cell of a grid of 3 x 2 has the list own,
 * (0, 0), right, bottom; a grid of one cell has own, (0, 0).
 * Candidates.  Walk the centres in list order; for each centre C take dy = -r..r ascending, then dx = -r..r ascending: v = C +
 * (dx, dy).  Duplicates are allowed.  r = 1 and the list (5, -3), (0, 0): (4, -4), (5, -4), (6, -4), (4, -3), .. (6, -2), (-1, -1),
 * (0, -1), .. (1, 1) -- walk index 4 is (5, -3), 9 is (-1, -1), 13 is (0, 0).
 * Cost.  With P = centre 0 as the predictor,
 *   J(v) = satd8x8(cur_block - ref_block_at(x + vx, y + vy)) + ((lambda_q4 * (L(vx - Px) + L(vy - Py))) >> 4)
 * where L(d) is the length of d as a signed Exp-Golomb code: k = 2 |d| - (d > 0), L = 2 floor(log2(k + 1)) + 1.  L(0) = 1,
 * L(1) = L(-1) = 3, L(2) = L(-2) = L(3) = L(-3) = 5, L(4) = 7, L(-7) = 7, L(8) = 9; |d| <= 16382 gives L <= 29, so J fits uint32.  With
 * lambda_q4 16 the predictor itself costs 2 beside its SATD, (Px + 1, Py) 4, (Px + 2, Py - 4) 12.
 * Winner.  The least J wins; among equal J the first candidate of the walk.  d_best[b] = {vx, vy, the winner's SATD (without the
 * vector cost)}; d_j[b] = its J.
 *
 * What follows from it:
 *   1. a zero seed with seed_scale 0, centres 0, lambda_q4 0 and range 8 gives bit for bit the d_best of xSatd8x8SearchFromTilesDev
 *      at range 8;
 *   2. range 0 with centres 0 gives the clamped seed and its SATD: for |seed << seed_scale| <= 8183 that is entry [49 b + 24] of
 *      xSatd8x8RefineQpelFromTilesGpu's d_costs for the same vector;
 *   3. a constant frame pair: every SATD ties, so with lambda_q4 0 the first entry of the walk wins, own + (-r, -r), and with
 *      lambda_q4 > 0 the predictor does.
 *
 * One host struct, read during the call; the pointers in it are device pointers (alignments: the field comments).  d_cur == d_ref
 * is allowed.  The outputs overlap nothing: in place (d_best == d_seed) is NOT allowed, blocks read their neighbours' seeds.  One
 * launch; the call allocates nothing, needs no xHipMeScratchReserve and can be captured into a graph; its result does not depend on
 * any launch option.  X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned
 * required buffer, a side that is not a positive multiple of 16, a scalar outside the range its field comment states, a span that
 * does not fit in the address space, and an output that overlaps any other buffer of the call.  The extents are width * height * 2
 * (d_cur, d_ref), 8 bytes per seed cell (d_seed), 8 bytes (d_best) and 4 bytes (d_j) per 8x8 block. */
typedef struct x266_seed_t {
    const x266_ref_block_t *d_cur;         /* [(width / 16) * (height / 16)], 16-byte aligned; only m_Y is read                 */
    const x266_ref_block_t *d_ref;         /* the same size, 16-byte aligned; only m_Y is read; may be d_cur                    */
    const x266_me_result_t *d_seed;        /* one per seed cell, 8-byte aligned; cost is ignored                                */
    x266_me_result_t *d_best;              /* [(width / 8) * (height / 8)], 8-byte aligned; output                              */
    uint32_t *d_j;                         /* one per 8x8 block or NULL, 4-byte aligned; output: the winner's J                 */
    int width, height;                     /* positive multiples of 16                                                          */
    int seed_scale;                        /* 0: a seed per 8x8 block, full-resolution samples; 1: per 16x16 tile, lowres ones  */
    int centres;                           /* 0..31, bits 0..4: add (0, 0), left, top, right, bottom                            */
    int range;                             /* r, 0..8                                                                           */
    int lambda_q4;                         /* 0..65535                                                                          */
} x266_seed_t;
int xSatd8x8SeededSearchGpu(x266hip_ctx *ctx, const x266_seed_t *p, void *stream);

/* ---- inter partition decision: merge the 8x8 vectors of a refined field into partitions of 16x16, 32x32 and 64x64 samples ----
 * The searches and the refinement leave one quarter-sample vector per 8x8 block.  This call decides, per CTU and bottom up, which
 * neighbouring blocks share a vector, by SATD plus vector bits, and returns again one x266_me_result_t per 8x8 block -- which
 * xMotionCompQpelGpu, xMotionCompBiQpelTiles and the deblocking calls take unchanged -- beside the partition's level per block (what a
 * host needs for the partition map and for the transform candidates of x266_tdecide_t.d_cand) and the price of every CTU.  No upstream
 * counterpart; the arithmetic here is the contract.
 *
 * Geometry.  width, height are positive multiples of 16; bw = width / 8, bh = height / 8; block b = by * bw + bx.  Level k = 0..3 has
 * nodes of n = 1 << k blocks a side (8, 16, 32, 64 samples) on the grid anchored at (0, 0): node (nx, ny) of level k covers blocks
 * X .. X + n - 1, Y .. Y + n - 1 with (X, Y) = (nx << k, ny << k).  A node is WHOLE if it lies inside the frame: nx < (bw >> k) and
 * ny < (bh >> k); every node of levels 0 and 1 is.  A node of level 2 or 3 that sticks out of the frame is CUT: it has no vector of its
 * own and always splits; its children that lie wholly outside the frame do not exist.  CTUs are the nodes of level 3, whole or cut,
 * ceil(width / 64) x ceil(height / 64) in raster order as in xTransformCtuFromTilesDev.
 * Input field.  d_mv holds one quarter-sample record per 8x8 block, the d_best of xSatd8x8RefineQpelFromTilesGpu; cost is ignored.
 * in(bx, by) = clamp(component, -32766, 32766).
 * Distortion.  D(b, q) = satd8x8(cur_b - P_q(b)) with P_q the luma prediction of xMotionCompQpelLumaGpu under the vector q: its edge
 * rule, filters and rounding.  D(node, q) is the sum of D(b, q) over the node's blocks.  There is no weighted prediction here.
 * Predictor of a node, from the INPUT field alone (nodes do not depend on each other's decisions): A = in(X - 1, Y), B = in(X, Y - 1),
 * C = in(X + n, Y - 1) if that block is inside the frame, else in(X - 1, Y - 1).  If exactly one of the three is inside the frame, P is
 * that one; otherwise P is the component-wise median of the three, a block outside the frame counting as (0, 0).
 * Rate and cost.  R(k, q) = (k > 0 ? 1 : 0) + L(qx - Px) + L(qy - Py) with L the signed Exp-Golomb length of xSatd8x8SeededSearchGpu
 * (L(0) = 1, L(1) = L(-1) = 3, ..), here of quarter-sample differences: |d| <= 65535, so L <= 33 and R <= 67.
 * Jw(node, q) = D(node, q) + ((lambda_q4 * R) >> 4); everything fits uint32.
 * Whole-node winners, bottom up and independent of the split decisions.  Level 0: W(b) = in(b).  For a whole node of level k >= 1, walk
 * its children in raster order (top left, top right, bottom left, bottom right); for each child vector W(child) take dy = -r..r
 * ascending, then dx = -r..r ascending: q = W(child) + (dx, dy) in quarter samples, each component then held to -32768..32767 (three
 * levels of +-1 around +-32766 would leave int16; only vectors far outside any frame reach this).  Duplicates are allowed.  The least Jw
 * wins, among equal values the first of the walk: W(node).
 * Decision, bottom up.  Best(level-0 node) = Jw(b, W(b)).  For a whole node of level k >= 1, S = the sum of Best over its children +
 * ((lambda_q4 * 1) >> 4); the node is ONE partition if Jw(node, W(node)) <= S (a tie merges) and Best = that Jw; otherwise it splits and
 * Best = S.  For a cut node Best is the sum of Best over its existing children, with no flag.
 * Outputs.  d_out[b] = the vector of the partition that contains b and D(b, that vector), the block's OWN 8x8 SATD.  d_level[b] = the
 * partition's level, 0..3.  d_ctu[c]: j = Best of the CTU; dist = the summed distortion of its partitions; bits = their summed R plus
 * one per whole node that split; parts = the number of partitions.  j is a sum of per-term floors -- one ">> 4" per partition and per
 * split flag -- and NOT dist + ((lambda_q4 * bits) >> 4).  d_nodes, if given, holds W(node) and cost = Jw(node, W(node)) of every whole
 * node: level 1 first, its (bw >> 1) * (bh >> 1) nodes in raster order, then level 2 ((bw >> 2) * (bh >> 2)), then level 3.
 *
 * Worked values.  A 32 x 32 frame (bw = bh = 4) with in(0, 0) = (4, -8), in(1, 0) = (12, -2), in(0, 1) = (3, 5), in(1, 1) = (-7, 9):
 * block (1, 0) has only A inside the frame, P = (4, -8); block (0, 1) has B = (4, -8) and C = (12, -2) inside and A outside, P =
 * (median(0, 4, 12), median(0, -8, -2)) = (4, -2); block (1, 1) has A = (3, 5), B = (12, -2) and C = in(2, 0); with in(2, 0) = (5, 1)
 * P = (5, 1).  The level-1 node at (X, Y) = (2, 2) has no block at (4, 1), so its C = in(1, 1).  With P = (4, -2) and lambda_q4 16,
 * q = (6, -2) at level 1 has R = 1 + L(2) + L(0) = 7 and Jw = D + 7; with lambda_q4 24, Jw = D + 10; q = P at level 0 has R = 2.
 *
 * What follows from it:
 *   1. with range 0 every output vector is an input vector (clamped) of the same CTU;
 *   2. with range 0, an input field with the same vector q in every block gives every whole CTU as one level-3 partition (the walk
 *      only meets q and a tie merges), cut CTUs their largest whole nodes, and the costs in d_out are the D(b, q) of
 *      xMotionCompQpelLumaGpu + xSatd8x8FromTilesDev -- at lambda_q4 0 and at every lambda_q4 >= 8.  Below 8 the per-term floors can
 *      favour the split by one: at lambda_q4 7 a node with P = q costs (7 * 3) >> 4 = 1 beside its SATD, its four children and the
 *      flag (7 * 2) >> 4 = 0 and 7 >> 4 = 0, so it splits;
 *   3. lambda_q4 0 and range 0: d_ctu[c].j <= the sum over the CTU's blocks of D(b, in(b));
 *   4. d_out through xMotionCompQpelLumaGpu and xSatd8x8FromTilesDev returns exactly the costs in d_out.
 *
 * One host struct, read during the call; the pointers in it are device pointers (alignments: the field comments).  d_cur == d_ref is
 * allowed.  The outputs overlap nothing: in place (d_out == d_mv) is NOT allowed, nodes read their neighbours' input vectors.  One
 * launch, one workgroup per CTU, no atomics: the same bytes on every run.  The call allocates nothing, needs no xHipMeScratchReserve
 * and can be captured into a graph; its result does not depend on any launch option.  X266HIP_EINVAL, with nothing launched and the
 * call named in xHipLastError: a NULL p, a NULL or misaligned required buffer, a misaligned d_nodes, a side that is not a positive
 * multiple of 16, a scalar outside the range its field comment states, a span that does not fit in the address space, and an output
 * that overlaps any other buffer of the call.  The extents are width * height * 2 (d_cur, d_ref), 8 bytes (d_mv, d_out) and 1 byte
 * (d_level) per 8x8 block, 16 bytes per CTU (d_ctu) and 8 bytes per whole node of levels 1..3 (d_nodes).  Offsets are size_t; frames
 * beyond 2^32 bytes are untested.
 * Out of scope: bi-directional partitions, weighted prediction, chroma in the cost, rectangular and ternary splits, merge and skip
 * candidates.  A predictor that follows the decided partitions in coding order, and the compact stream of the decided field, are
 * xMotionPackGpu's (below). */
typedef struct x266_part_ctu_t {
    uint32_t j;            /* Best of the CTU: a sum of per-term floors                                     */
    uint32_t dist;         /* the summed distortion of its partitions                                       */
    uint32_t bits;         /* their summed R plus one per whole node that split                             */
    uint32_t parts;        /* the number of partitions                                                      */
} x266_part_ctu_t;         /* 16 bytes */
typedef struct x266_part_t {
    const x266_ref_block_t *d_cur;         /* [(width / 16) * (height / 16)], 16-byte aligned; only m_Y is read                 */
    const x266_ref_block_t *d_ref;         /* the same size, 16-byte aligned; only m_Y is read; may be d_cur                    */
    const x266_me_result_t *d_mv;          /* [(width / 8) * (height / 8)], 8-byte aligned; quarter samples; cost is ignored    */
    x266_me_result_t *d_out;               /* one per 8x8 block, 8-byte aligned; output                                         */
    uint8_t *d_level;                      /* one per 8x8 block, 1-byte aligned; output: the partition's level, 0..3            */
    x266_part_ctu_t *d_ctu;                /* one per CTU, 8-byte aligned; output                                               */
    x266_me_result_t *d_nodes;             /* one per whole node of levels 1..3 or NULL, 8-byte aligned; output                 */
    int width, height;                     /* positive multiples of 16                                                          */
    int range;                             /* r, 0..1                                                                           */
    int lambda_q4;                         /* 0..65535                                                                          */
} x266_part_t;
int xInterPartitionDecideGpu(x266hip_ctx *ctx, const x266_part_t *p, void *stream);

/* ---- the compact motion stream: the decided field as a per-CTU stream for the host's entropy coder, and back ----
 * xInterPartitionDecideGpu leaves its decision dense: 8 + 1 bytes per 8x8 block, although a frame is a few thousand partitions.
 * xMotionPackGpu turns d_out and d_level into one 32-byte record per CTU and four 16-bit words per partition in coding order, the
 * differences formed against a predictor a decoder can reproduce; xMotionUnpackGpu is the exact inverse on the vectors and levels and the
 * entry of a decoder into xMotionCompQpelGpu.  No upstream counterpart; the arithmetic here is the contract.
 *
 * Geometry.  width, height, bw, bh, the levels, the nodes and which of them are WHOLE, CUT or do not exist, and the CTUs in raster
 * order: exactly as the inter partition decision states them (above).  n_ctu = ceil(width / 64) * ceil(height / 64).  Inside a CTU the
 * block at (x, y), each 0..7 relative to the CTU's first block, has the Morton index i = 0..63: bit 2b of i is bit b of x and bit
 * 2b + 1 of i is bit b of y (i = 0, 1, 2, 3 are (0,0), (1,0), (0,1), (1,1); i = 4 is (2,0)).  A node of level k is the 4^k consecutive
 * indices from a multiple of 4^k.
 * Coding order: CTUs in raster order; inside a CTU the quadtree walk top left, top right, bottom left, bottom right -- which visits
 * the partitions in ascending Morton index of their first block.
 *
 * Partitions as pack sees them.  Pack trusts only first blocks.  It walks each CTU from level 3 down: the node of level k whose first
 * block is (X, Y) is ONE partition if it is whole and (d_level[Y * bw + X] & 3) >= k; otherwise it splits into its existing children.
 * A cut node always splits; level 0 always ends the walk.  The partition's vector q is d_mv[Y * bw + X], the full int16 range, no
 * clamp.  So a field that is not constant inside its partitions, and level bytes with high bits set or that disagree inside a
 * partition, are legal input: pack canonicalises them to what the first blocks say.  (A predictor that reads such a block -- below, it
 * reads d_mv where it stands -- cannot be reproduced by a decoder, which only ever sees the canonical field: differences are decodable
 * for fields that are constant inside their partitions, which is what xInterPartitionDecideGpu emits.)
 * The head mask.  head_mask has bit i set when block i is the first block of a partition.  A reader recovers the level of head h from
 * the mask and the geometry: the largest k for which h is a multiple of 4^k, the node of level k at h is whole, and no other mask bit
 * lies in (h, h + 4^k).
 *
 * Causal predictor.  The predictor of a partition of n = 1 << k blocks a side at (X, Y) reads d_mv at the blocks A = (X - 1, Y),
 * B = (X, Y - 1), and C = (X + n, Y - 1) if that block is inside the frame AND precedes the partition in coding order -- its CTU's
 * raster index is lower, or it lies in the same CTU with a Morton index below the head's --, otherwise C = (X - 1, Y - 1).  A, B and
 * (X - 1, Y - 1) always precede.  If exactly one of the three is inside the frame, P is that one; otherwise P is the component-wise
 * median of the three, a block outside the frame counting as (0, 0): the rule of the partition decision, on other blocks and without
 * its clamp.
 * Differences, payload and bits.  The true difference is d = q - P in int32, |d| <= 65535.  The payload of a partition is 4 words:
 * qx, qy, then the low 16 bits of dx and of dy.  A decoder recovers q = (int16_t)(P + (int16_t)word): P + (int16_t)word and q differ
 * by a multiple of 65536, q fits int16, and the cast keeps exactly the low 16 bits -- so the result is q whatever |d| was.  The payload of
 * a CTU is its partitions in coding order, d_stream[offset .. offset + n_words).  bits = the sum over the CTU's partitions of
 * (k > 0 ? 1 : 0) + L(dx) + L(dy), plus one per whole node that split; L is the signed Exp-Golomb length of xSatd8x8SeededSearchGpu
 * (xMotionVectorBits: L(0) = 1, L(+-1) = 3, L(+-65535) = 33).  This is the accounting of x266_part_ctu_t.bits under the causal predictor,
 * so the two are comparable.  max_abs is the largest |dx| or |dy| of the CTU.
 *
 * Worked values.  A 32 x 32 frame (bw = bh = 4) that is all level 1 has the heads 0, 4, 8 and 12 at the blocks (0,0), (2,0), (0,2) and
 * (2,2), head_mask 0x1111, parts 4, n_words 16.  The partition at (0,2) has C = block (2,1): its Morton index 6 is below 8, it is
 * available.  The partition at (2,2) has (4,1) outside the frame, so C = (1,1).  Were (1,1) a level-0 block, Morton 3, its above-right
 * (2,0) is Morton 4 and not yet coded, so its C = (0,0) -- the decision's own predictor would have used in(2,0) there.
 *
 * Offsets and capacity.  offset[c] is the exclusive prefix sum of n_words over the CTUs before c, in 64 bits, a multiple of 4.
 * xMotionPackGpu writes every record.  d_total[0] = the total number of words, d_total[1] = the number of leading CTUs whose payload
 * lies completely inside cap_words (n_ctu exactly when the stream fits).  The payload of CTU c is written if and only if offset +
 * n_words <= cap_words; no word at or beyond cap_words is ever written.  cap_words == 0 with d_stream == NULL is the count-only call:
 * records and totals to size a buffer with.  Three launches on the caller's stream: count and records, the offsets (the scan of
 * xLevelsPackGpu, xLevelsScanChunk() records per step), write.
 *
 * xMotionUnpackGpu trusts nothing in a record but head_mask and offset.  A mask is well formed if bit 0 is set, no bit of a block that
 * does not exist is set, and every existing block i lies in [h, h + 4^level(h)) of the largest head h <= i.  A CTU whose mask is
 * malformed, or with offset + 4 * popcount(head_mask) > cap_words (computed without overflow), is written as vector (0, 0), cost 0,
 * level 0 in all its existing blocks.  Otherwise every block gets its partition's (qx, qy), cost 0 and level.  Words 2 and 3 of a
 * partition are not read; nothing outside [0, cap_words) of the stream is ever read: the stream comes from a host decoder, and offset
 * needs no alignment there.  d_total is ignored; d_stream may be NULL when cap_words == 0.  One launch.
 *
 * Both calls take one host struct, read during the call; the pointers in it are device pointers (alignments: the field comments).
 * One wave per CTU, no atomics: the same input gives the same bytes on every run.  Neither call allocates; both can be captured into a
 * graph; the result depends on no launch option.  X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a
 * NULL or misaligned required buffer, a side that is not a positive multiple of 16, a span that does not fit in the address space, an
 * output overlapping any other buffer of the call.  The extents are 8 bytes (d_mv) and 1 byte (d_level) per 8x8 block, 32 bytes per CTU
 * (d_ctu), cap_words * 2 (d_stream) and 16 bytes (d_total).  Offsets are size_t; frames beyond 2^32 bytes are untested.
 * Out of scope: bi-directional and intra blocks in the stream, merge and skip candidates.  Binarisation and coding of the stream are
 * xEntropyEncodeMvGpu's, the device-side reconstruction of the vectors from the differences is xMotionReconstructGpu's (both below;
 * xMotionPredictor covers the latter on the host). */
typedef struct x266_motion_ctu_t {   /* 32 bytes; the first 20 bytes are laid out as x266_level_region_t's */
    uint64_t head_mask;  /* bit i set: block i of the CTU (Morton index) starts a partition  */
    uint64_t offset;     /* start of the CTU's payload in d_stream, in 16-bit words          */
    uint32_t n_words;    /* 4 * parts                                                        */
    uint32_t parts;      /* popcount(head_mask)                                              */
    uint32_t bits;       /* flags + Exp-Golomb bits of the differences                       */
    uint32_t max_abs;    /* largest |true difference component| of the CTU, 0..65535         */
} x266_motion_ctu_t;
typedef struct x266_motion_t {
    x266_me_result_t *d_mv;      /* [bw * bh], 8-byte aligned; pack reads, unpack writes (cost = 0)              */
    uint8_t *d_level;            /* [bw * bh], any alignment; pack reads (value & 3), unpack writes              */
    x266_motion_ctu_t *d_ctu;    /* [n_ctu], 8-byte aligned; pack writes, unpack reads                           */
    uint16_t *d_stream;          /* [cap_words], 16-byte aligned; pack writes, unpack reads                      */
    uint64_t *d_total;           /* [2], 8-byte aligned; pack writes {words, leading CTUs that fit}; unpack ignores (may be NULL there) */
    int width, height;           /* positive multiples of 16 */
    uint64_t cap_words;
} x266_motion_t;
int xMotionPackGpu  (x266hip_ctx *ctx, const x266_motion_t *p, void *stream);
int xMotionUnpackGpu(x266hip_ctx *ctx, const x266_motion_t *p, void *stream);
/* Host only, the functions the kernels run.  xMotionWalk: the partitions of CTU `ctu` of a width x height frame under head_mask, in coding
 * order: head[j] the Morton index of the first block and level[j] the level of partition j < the return value, the other entries 0;
 * X266HIP_EINVAL for a malformed mask (as xMotionUnpackGpu judges it), a bad size, a ctu >= n_ctu or a NULL array.  xMotionPredictor: the
 * causal predictor p of the whole node of `level` at block (X, Y) from a host copy of the field ([bw * bh], only mvx and mvy are read);
 * X266HIP_EINVAL for a bad size, a NULL pointer, a level outside 0..3 or an (X, Y) that is not the first block of a whole node of that
 * level.  xMotionVectorBits: L(d) for |d| <= 65535, else -1. */
int xMotionWalk(int width, int height, size_t ctu, uint64_t head_mask, uint8_t head[64], uint8_t level[64]);
int xMotionPredictor(int width, int height, const x266_me_result_t *field, int X, int Y, int level, int16_t p[2]);
int xMotionVectorBits(int d);

/* ---- the entropy coder: the levels as a range-coded byte stream, one independent substream per 32x32 region, and back ----
 * xLevelsPackGpu hands words to a host coder; xRdoQuantRegionsGpu, xTransformDecideCtuTilesGpu and xLevelsBitsGpu optimise against a
 * static rate model.  xEntropyEncodeLevelsGpu codes the levels themselves, on the device, with an adaptive binary range coder whose
 * syntax mirrors that model term by term, so that estimate and bytes can be compared; xEntropyDecodeLevelsGpu is the exact inverse and
 * the entry of a decoder into xQuantRegionsGpu(1).  No upstream counterpart; the arithmetic here is the contract.
 *
 * Region, class byte, block layout, scan, CGs and CG bit g: exactly as the compact level stream states them (xLevelsPackGpu,
 * xLevelScan).  N = 4 << (class & 3), n = log2 N; d_class == NULL: N = 32.  pos(), g, rem() and the position class are the rate
 * model's (xRdoQuantRegionsGpu).
 *
 * Syntax of a region.  Its (32 / N)^2 blocks in raster order; per block:
 *     cbf                             one bin: the block has a non-zero level.  If 0 the block ends here.
 *     last position p = (u_p, v_p)    the last non-zero scan position, u_p first, then v_p.  A coordinate t: its group index g (g = t for
 *                                     t < 4, otherwise 2 ilog2(t) + ((t >> (ilog2(t) - 1)) & 1)) as g one-bins and, if g < 2n - 1, a
 *                                     zero-bin: min(g + 1, 2n - 1) bins, bin i coded with context (x or y, i).  For g >= 4 then the
 *                                     (g >> 1) - 1 low bits of t as bypass bins, most significant first.
 *     the CGs s = 0 .. s_p in ascending scan order, s_p the CG of p:
 *         cgf                         for 0 < s < s_p only: the CG has a non-zero level.  If 0 the CG ends here.  CG 0 and CG s_p are
 *                                     implied coded (CG 0 even when it holds no level).
 *         the positions i of the CG in ascending scan order, in CG s_p only those up to p:
 *             sig                     the level is non-zero; context = the position class (0, 1 or 2).  Not coded for p itself.
 *             for a non-zero level l: gt1 (|l| > 1); if set gt2 (|l| > 2); if set the remainder r = |l| - 3 in bypass bins: min(r, 3)
 *                                     ones, then a zero if r < 3, otherwise Exp-Golomb order 0 of r - 3 (with v = r - 2 and k =
 *                                     ilog2(v): k ones, a zero, the k low bits of v, most significant first); rem(r) bins in all.
 *                                     Then the sign as a bypass bin, 1 = negative.  All bins of one coefficient stay together.
 * The level -32768 is legal: magnitude 32768, r = 32765, k = 14.
 * Decoded positions cannot leave the block: a coordinate's prefix stops at g = 2n - 1, and for g >= 4 the decoder forms t =
 * ((2 + (g & 1)) << ((g >> 1) - 1)) | suffix with (g >> 1) <= n - 1, so t < 2^n; for n = 2, t = g <= 3.  Every (u, v) below N names one
 * scan position of the block.
 *
 * Contexts.  Per block size 25, in this order: cbf; last x, bin 0..8; last y, bin 0..8; cgf; sig of class 0, 1, 2; gt1; gt2.  The
 * table is 4 x 25 = X266_ENTROPY_CONTEXTS entries, size 4 first.  A context is the probability p of a ZERO bin in 1/2048, 11 bits.
 * Every region starts from the call's initial table: regions are independent substreams, and nothing adapted ever leaves a region.
 * The initial table `init` is HOST memory, 100 uint16, read during the call and passed to the kernels by value; every entry must lie
 * in 31 .. 2017 (the interval the adaptation below never leaves).  NULL is the default table (xEntropyDefaultInit): from the model's
 * costs c0, c1 of a zero and a one in 1/16 bit, p = 2048 * 2^(-c0/16) / (2^(-c0/16) + 2^(-c1/16)) rounded to nearest and held to 31 ..
 * 2017; 1024 for cbf (the model has no term) and for the last-position prefix (16 per bin).  Per size: 19 x 1024, then cgf 1385, sig
 * 723 1242 1609, gt1 1325, gt2 1263.  A host may pass any table; the decoder must take the same one.  Neither call accepts or returns
 * adapted tables.
 *
 * Coder: the LZMA range coder, as recalled.  range is 32 bits and starts at 0xFFFFFFFF; low is a mathematical integer that starts at 0
 * (an implementation keeps 33 bits of it, a cache byte and a count of pending 0xFF bytes for the carry).
 *     context bin b with probability p:  bound = (range >> 11) * p.   b = 0: range = bound, p += (2048 - p) >> 5.
 *                                                                    b = 1: low += bound, range -= bound, p -= p >> 5.
 *     bypass bin b:                      range >>= 1; if b: low += range.
 *     after every bin, while range < 2^24:  range <<= 8, low <<= 8 (one byte leaves; with p in 31 .. 2017 this happens at most once).
 *     termination:                       low = (low + 0xFFFFFF) & ~0xFFFFFF, then five more byte shifts.
 * The bytes are low, big endian.  The leading byte -- always 0, a carry never reaches it -- is not stored, and trailing zero bytes are
 * not stored (after the termination's rounding at least the last three are zero).  n_bytes counts what is stored.  The decoder starts
 * with range = 0xFFFFFFFF and code = the first four stored bytes, reads 0 beyond the end of a substream, and for a context bin takes b
 * = 0 iff code < bound (otherwise code -= bound), for a bypass bin b = 1 iff code >= range after the halving (then code -= range); it
 * renormalises with code = (code << 8 | next byte); all in 32-bit unsigned arithmetic.  So an all-zero region is 0 bytes, and a
 * region's overhead over its information is one or two bytes, not five.
 * Worked values, 32x32 regions under the default table, bytes in hex.  The only level DC = 1: 80 (4 context bins, 1 bypass bin; one
 * word, 0x0080).  The only level DC = -32768: 9f ff fa ea cd (5 and 33 bins).  The only level a 3 at index 1023, the last scan position:
 * ff ff ff 7e fb 80 04 12 (114 and 8 bins).
 * The largest substream.  A region has at most 3456 context bins (64 blocks of 4x4: 1 + 6 + 15 + 32 each) and at most 33 824 bypass bins
 * (1024 levels of rem(32765) + 1 = 33 bins, and 32 last-position suffix bits at 8x8).  A context bin shrinks the range by no less than
 * 31/2048 less the truncation of range >> 11, under 6.05 bits; a bypass bin costs under 1.0001 bits.  That is under 54 740 bits, no
 * more than 6843 byte shifts, and with the termination 6847 bytes: X266_ENTROPY_MAX_BYTES = 6848, 3424 words.  (All 1024 levels at
 * +-32767 under a table of 2017s come to 4342 bytes; the bound is the floor's, not a measured one.)
 *
 * Stream and records.  d_stream is in 16-bit words, little endian: byte j of a substream is bits 8 (j & 1) .. of word offset + j / 2.  A
 * substream of odd length is padded with one zero byte; n_words = (n_bytes + 1) / 2.  Per region one 32-byte record whose first 20 bytes
 * are laid out as x266_level_region_t's.  offset[r] is the exclusive prefix sum of n_words, in 64 bits.
 * xEntropyEncodeLevelsGpu writes every record.  d_total[0] = the total number of words, d_total[1] = the number of leading regions whose
 * payload lies completely inside cap_words (n_regions exactly when the stream fits).  The payload of region r is written if and only if
 * offset + n_words <= cap_words; no word at or beyond cap_words is ever written.  cap_words == 0 with d_stream == NULL is the count-only
 * call: records and totals to size a buffer with.  With d_nnz != NULL a region with d_nnz[r] == 0 counts as all zero and its levels are
 * not read.  n_regions == 0 writes d_total = {0, 0} and nothing else.  Three launches on the caller's stream: count and records, the
 * offsets (the scan of xLevelsPackGpu, xLevelsScanChunk() records per step), write.  One wave per region; no atomics, no allocation; the
 * same input gives the same bytes on every run and under every launch option; the call can be captured into a graph.
 *
 * xEntropyDecodeLevelsGpu trusts nothing in a record but offset and n_bytes, and holds both against cap_words before any load: a region
 * with offset > cap_words, (n_bytes + 1) / 2 > cap_words - offset or n_bytes > X266_ENTROPY_MAX_BYTES is written as all zero with
 * d_nnz[r] = 0.  Nothing outside [0, cap_words) of the stream is ever read, and inside a substream only its n_bytes count.  Decoding is
 * total: every loop of the syntax is bounded, so any bytes decode to some region or are malformed.  Malformed: an Exp-Golomb prefix
 * longer than 14, a magnitude above 32768, the value +32768.  A malformed region is written as all zero with d_nnz[r] = 0.  Otherwise all
 * 1024 levels are written, absent ones as zeros, and with d_nnz != NULL the non-zero count.  (A decoded region may hold a coded CG
 * without a level or a last position at a zero CG 0 only through garbage; re-encoding it gives the canonical bytes.)  d_total is
 * ignored; d_stream may be NULL when cap_words == 0.  One launch.
 *
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned required buffer, a NULL
 * d_stream with cap_words != 0, an entry of init outside 31 .. 2017, a span that does not fit in the address space, an output
 * overlapping any other buffer.  The extents are the compact level stream's, with n_regions * 32 for d_region.  With n_regions == 0
 * only d_total of the encode call is looked at.
 * Out of scope, the follow-ups (per-frame context statistics are xEntropyStatsLevelsGpu's, below): context carry-over between regions, WPP-style rows included; sign hiding and dependent quantisation; splitting
 * a region's blocks over lanes as separate coders (a format question: separate coders are separate substreams); any real VVC or HEVC
 * bit-stream syntax.  Class bytes, intra modes, kinds and qp are not in this substream: the motion stream is xEntropyEncodeMvGpu's and the
 * side information xEntropyEncodeSideGpu's (both below).  A "bitrate" from these two calls is the residual's alone; the three coders
 * together hold what a P-frame needs, and until contexts carry over their bytes are an upper estimate of a real stream's. */
#define X266_ENTROPY_CONTEXTS  100
#define X266_ENTROPY_MAX_BYTES 6848
typedef struct x266_entropy_region_t {   /* 32 bytes; the first 20 bytes are laid out as x266_level_region_t's */
    uint32_t ctx_bins;     /* context-coded bins of the region                                   */
    uint32_t bypass_bins;  /* bypass bins of the region                                          */
    uint64_t offset;       /* start of the region's substream in d_stream, in 16-bit words       */
    uint32_t n_words;      /* (n_bytes + 1) / 2                                                  */
    uint32_t n_bytes;      /* bytes of the substream, 0 .. X266_ENTROPY_MAX_BYTES                */
    uint32_t n_nz;         /* non-zero levels of the region (what d_nnz holds)                   */
    uint32_t reserved;     /* written 0                                                          */
} x266_entropy_region_t;
typedef struct x266_entropy_t {
    int16_t  *d_level;                 /* [n_regions * 1024], 16-byte aligned; encode reads, decode writes            */
    const uint8_t *d_class;            /* [n_regions] or NULL (every region 32x32), any alignment                     */
    uint32_t *d_nnz;                   /* [n_regions] or NULL, 4-byte aligned; encode reads, decode writes (above)    */
    x266_entropy_region_t *d_region;   /* [n_regions], 8-byte aligned; encode writes, decode reads                    */
    uint16_t *d_stream;                /* [cap_words], 16-byte aligned; encode writes, decode reads                   */
    uint64_t *d_total;                 /* [2], 8-byte aligned; encode writes, decode ignores (may be NULL there)      */
    const uint16_t *init;              /* HOST memory, [X266_ENTROPY_CONTEXTS], or NULL: the default table            */
    size_t    n_regions;
    uint64_t  cap_words;
} x266_entropy_t;
int xEntropyEncodeLevelsGpu(x266hip_ctx *ctx, const x266_entropy_t *p, void *stream);
int xEntropyDecodeLevelsGpu(x266hip_ctx *ctx, const x266_entropy_t *p, void *stream);
/* Host only, the functions the kernels run.  xEntropyDefaultInit writes the default table.  xEntropyEncodeRegion codes the 1024 levels of
 * one region of class `cls` (only cls & 3 counts) from `init` (NULL: the default): it returns n_bytes, stores the first min(n_bytes, cap)
 * bytes in out (which may be NULL with cap 0) and, with bins != NULL, the context and the bypass bin counts.  xEntropyDecodeRegion
 * writes all 1024 levels and, with n_nz != NULL, the count; it returns 0, or 1 for a malformed substream (then zeros).  Both return
 * X266HIP_EINVAL for a NULL level array, a NULL buffer with a length, a table entry outside 31 .. 2017 or an n_bytes above
 * X266_ENTROPY_MAX_BYTES. */
int xEntropyDefaultInit(uint16_t init[X266_ENTROPY_CONTEXTS]);
int xEntropyEncodeRegion(const int16_t *level, int cls, const uint16_t *init, uint8_t *out, size_t cap, uint32_t bins[2]);
int xEntropyDecodeRegion(const uint8_t *bytes, size_t n_bytes, int cls, const uint16_t *init, int16_t *level, uint32_t *n_nz);

/* ---- the entropy coder of the motion stream: range-coded CTU substreams, and the vectors rebuilt from the differences ----
 * xMotionPackGpu leaves the motion field as 16-bit words for a host coder, and xMotionUnpackGpu reads the vectors themselves, which a bit
 * stream does not carry.  xEntropyEncodeMvGpu codes the quadtree and the differences of pack's stream on the device, one independent
 * substream per CTU under the range coder of the levels (above; the coder, its bytes, the stream's words and the padding are exactly
 * those); xEntropyDecodeMvGpu is its inverse and writes a stream of pack's form with the vectors left out; xMotionReconstructGpu
 * rebuilds the dense field from the differences on the device.  No upstream counterpart; the arithmetic here is the contract.
 *
 * Geometry, Morton index, nodes (WHOLE, CUT, not existing), head mask, level of a head, well-formedness of a mask, causal predictor and
 * the payload of a partition: exactly as the compact motion stream states them (xMotionPackGpu).
 *
 * Syntax of a CTU.  The payload is the quadtree, and the vectors are coded where the walk reaches them.  Visit the level-3 node of the
 * CTU; for a node of level k whose first block is h:
 *     the node does not exist (h is outside the frame)   nothing
 *     k == 0                                             a partition
 *     the node is CUT                                    no bin; visit its four children top left, top right, bottom left, bottom right
 *     the node is WHOLE                                  one bin `split` with context split[k]: 0 = the node is one partition, 1 = visit
 *                                                        its four children in the same order
 * A partition codes dx, then dy: the TRUE differences, |d| <= 65535.  The encoder has qx, qy and the low 16 bits w of each difference
 * in pack's words: P = (int16_t)(q - (int16_t)w) and d = q - P, exact by the argument of the pack section.  One component d:
 *     nz     d != 0, context per component.  If 0 the component ends here.
 *     gt1    |d| > 1, context per component.
 *     if set: r = |d| - 2 in bypass bins as Exp-Golomb order 1: with v = r + 2 and k = ilog2(v) >= 1, k - 1 ones, a zero, then the k low
 *            bits of v, most significant first.  r <= 65533, so v <= 65535, k <= 15: at most 30 bins.
 *     sign   a bypass bin, 1 = negative.
 * Contexts.  X266_ENTROPY_MOTION_CONTEXTS = 7, in this order: split of level 1, 2, 3; nz of x, of y; gt1 of x, of y.  They restart at
 * every CTU from the call's table: CTUs are independent substreams.  `init` is HOST memory, 7 uint16 in 31 .. 2017, read during the call
 * and passed by value; NULL is the default table (xEntropyMvDefaultInit), all 1024: the estimate this syntax mirrors
 * (xMotionVectorBits, one bit per flag) has no skew.
 * Bins against bits.  L(d) is 1 for d = 0, 3 for |d| = 1 and 2 ilog2(|d|) + 3 above (k = 2|d| - (d > 0) has ilog2(k + 1) = ilog2(|d|) +
 * 1 for |d| >= 1); the component's bins are 1, 3 and 2 ilog2(|d|) + 3: the same.  The flags are one bin each.  So for every readable
 * CTU ctx_bins + bypass_bins == x266_motion_ctu_t.bits exactly, and the coded bytes are that estimate made adaptive.
 *
 * Decoder rules.  Every loop is bounded (64 blocks, 3 levels, 15 prefix bins, 15 suffix bits).  The only malformed case is an
 * Exp-Golomb prefix of more than 14 ones; a well-formed prefix gives v <= 65535, so |d| <= 65535 always.  The decoder puts out the low 16
 * bits of d.  The mask it builds is well formed by construction.
 * The empty substream and the flat CTU.  Zero bytes decode, under every table, to the FLAT CTU: every whole node unsplit wherever the
 * cut nodes above it lead, every difference zero (all its bins are zero bins, and a decoder that reads zeros takes the zero side of
 * every context bin).  The flat CTU also encodes to zero bytes: a still CTU costs nothing.  This one rule covers every failure:
 *     on encode  a CTU whose mask is malformed (as xMotionUnpackGpu judges it) or with offset + 4 * popcount(head_mask) > in_words
 *                (computed without overflow) is coded as the empty substream; its record says parts = 0, unreadable = 1 and no bins.
 *     on decode  a record with offset > cap_words, (n_bytes + 1) / 2 > cap_words - offset or n_bytes > X266_ENTROPY_MOTION_MAX_BYTES
 *                decodes as the empty substream (d_status 1); a malformed substream gives the flat CTU as well (d_status 2).
 * Nothing outside [0, cap_words) of d_stream, respectively [0, in_words) of d_words, is ever read.
 *
 * The largest substream.  At most 21 split bins (1 + 4 + 16) and 64 partitions x 4 = 277 context bins, each under 6.05 bits (the level
 * coder's bound), and at most 64 x 2 x 31 = 3968 bypass bins, each under 1.0001 bits: under 5645 bits, no more than 706 byte shifts, and
 * with the termination 710 bytes.  X266_ENTROPY_MOTION_MAX_BYTES = 720, a multiple of 16 for the staging slab.  (64 level-0 partitions
 * with every |d| = 65535 come to 511 bytes under the default table; the bound is the floor's, not a measured one.)
 *
 * Worked values, under the default table, bytes in hex (context bins, bypass bins):
 *     64 x 64, one level-3 partition, d = (0, 0):               no bytes (3, 0)
 *     64 x 64, one level-3 partition, d = (1, 0):               40 (4, 1)
 *     64 x 64, one level-3 partition, d = (-2, 5):              67 90 (5, 8)
 *     64 x 64, one level-3 partition, d = (-65535, 65535):      7f ff bb ff ff ff df ff c0 (5, 62)
 *     32 x 32, all level 1 (heads 0, 4, 8, 12; level 3 is cut, level 2 is whole and splits),
 *              d in coding order (4, -8), (0, 0), (-1, 1), (0, 3):   b8 78 3e d0 c2 (18, 17)
 *     16 x 16, four level-0 blocks (levels 3 and 2 are cut), all d = 0:   80 (9, 0)
 *     16 x 16, one level-1 partition, d = 0 (the flat CTU):     no bytes (3, 0)
 *
 * xEntropyEncodeMvGpu reads d_ctu[c].head_mask and offset and the words d_words[offset .. offset + 4 * popcount) of pack's stream
 * (offset needs no alignment), and writes every record of d_coded.  offset there is the exclusive prefix sum of n_words, in 64 bits;
 * d_total[0] = the total number of words, d_total[1] = the number of leading CTUs whose substream lies completely inside cap_words.  A
 * substream is written if and only if offset + n_words <= cap_words; no word at or beyond cap_words is ever written.  cap_words == 0
 * with d_stream == NULL is the count-only call.  Three launches on the caller's stream: count and records, the offsets (the scan of
 * xLevelsPackGpu), write.
 * xEntropyDecodeMvGpu trusts nothing in a record of d_coded but offset and n_bytes, and holds both against cap_words before any
 * load.  CTU c's payload goes to the fixed place d_words[256 c ..): per partition the words 0, 0, low16(dx), low16(dy); words of
 * [256 c, 256 c + 256) beyond the payload are not written.  It writes every field of d_ctu[c]: head_mask, offset = 256 c, n_words =
 * 4 * parts, parts, and bits and max_abs recomputed from the decoded true differences.  For an encoder's input that came from
 * xMotionPackGpu, decode of encode returns pack's records in every field but offset, and pack's words 2 and 3.  d_status, if not NULL,
 * gets 0 (good), 1 (record outside the capacity) or 2 (malformed substream) per CTU.  d_total is ignored; d_stream may be NULL when
 * cap_words == 0; in_words is ignored.  One launch.
 * Both: one wave per CTU, the coder's chain on one lane over LDS; no atomics, no allocation; the same input gives the same bytes on
 * every run and under every launch option; the calls can be captured into a graph.
 *
 * xMotionReconstructGpu takes x266_motion_t as it is: xMotionUnpackGpu for a stream whose words 0 and 1 are not to be trusted.  It
 * reads d_ctu[c].head_mask, offset and the words 2 and 3 of each partition -- words 0 and 1 are never read, nor anything outside
 * [0, cap_words) -- and writes d_mv (cost 0) and d_level for every existing block.  Per partition in coding order q = (int16_t)(P +
 * (int16_t)word), P the causal predictor over the field as reconstructed so far.  A CTU whose mask is malformed or whose payload does
 * not lie inside cap_words is written as vector (0, 0), level 0, exactly as unpack writes it; later CTUs predict from those zeros, so
 * the result is a function of the input alone.  d_total is ignored; the X266HIP_EINVAL rules and the extents are unpack's.
 * Schedule.  CTU (cx, cy) reads the CTUs to its left, above, above left and above RIGHT (C of a partition that touches the CTU's top
 * right corner), so it belongs to step cx + 2 cy of cw + 2 (ch - 1) steps: one launch per step on the caller's stream, one wave per
 * CTU of the step, ordered by the stream alone -- no flags, no waiting on memory, no cooperative launch.
 *
 * X266HIP_EINVAL for the two coder calls, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned
 * required buffer (alignments: the field comments), a NULL d_stream with cap_words != 0, an entry of init outside 31 .. 2017, a side
 * that is not a positive multiple of 16, a span that does not fit in the address space, an output overlapping any other buffer.  The
 * extents are 32 bytes per CTU for d_ctu and for d_coded, in_words * 2 (encode) or 512 bytes per CTU (decode) for d_words, cap_words * 2
 * for d_stream, 16 bytes for d_total and one byte per CTU for d_status.  On encode d_words may be NULL when in_words == 0.
 * Out of scope: class bytes, intra modes, kinds and qp (they travel in the side stream, xEntropyEncodeSideGpu, below); context carry-over
 * between CTUs; adapted tables coming back from the device;
 * bi-directional fields; merge and skip candidates; a persistent or flag-synchronised wavefront kernel. */
#define X266_ENTROPY_MOTION_CONTEXTS  7
#define X266_ENTROPY_MOTION_MAX_BYTES 720
typedef struct x266_entropy_motion_ctu_t {   /* 32 bytes; the first 20 bytes are laid out as x266_level_region_t's */
    uint32_t ctx_bins;     /* context-coded bins of the CTU                                      */
    uint32_t bypass_bins;  /* bypass bins of the CTU                                             */
    uint64_t offset;       /* start of the CTU's substream in d_stream, in 16-bit words          */
    uint32_t n_words;      /* (n_bytes + 1) / 2                                                  */
    uint32_t n_bytes;      /* bytes of the substream, 0 .. X266_ENTROPY_MOTION_MAX_BYTES         */
    uint32_t parts;        /* partitions coded; 0 for an unreadable CTU                          */
    uint32_t unreadable;   /* 1: the input CTU could not be read and was coded as the empty substream */
} x266_entropy_motion_ctu_t;
typedef struct x266_entropy_motion_t {
    x266_motion_ctu_t *d_ctu;            /* [n_ctu], 8-byte aligned; encode reads head_mask and offset only, decode writes every field */
    uint16_t *d_words;                   /* 16-byte aligned; encode reads pack's stream, [in_words]; decode writes [256 * n_ctu]       */
    x266_entropy_motion_ctu_t *d_coded;  /* [n_ctu], 8-byte aligned; encode writes, decode reads offset and n_bytes only              */
    uint16_t *d_stream;                  /* [cap_words], 16-byte aligned; the coded bytes, little-endian words as the level coder's   */
    uint64_t *d_total;                   /* [2], 8-byte aligned; encode writes {words, leading CTUs that fit}; decode ignores (may be NULL there) */
    uint8_t  *d_status;                  /* [n_ctu] or NULL, any alignment; decode only: 0 good, 1 record outside the capacity, 2 malformed substream */
    const uint16_t *init;                /* HOST memory, [X266_ENTROPY_MOTION_CONTEXTS], or NULL: the default table                   */
    int width, height;                   /* positive multiples of 16 */
    uint64_t in_words, cap_words;
} x266_entropy_motion_t;
int xEntropyEncodeMvGpu(x266hip_ctx *ctx, const x266_entropy_motion_t *p, void *stream);
int xEntropyDecodeMvGpu(x266hip_ctx *ctx, const x266_entropy_motion_t *p, void *stream);
int xMotionReconstructGpu  (x266hip_ctx *ctx, const x266_motion_t *p, void *stream);
/* Host only, the functions the kernels run.  xEntropyMvDefaultInit writes the default table.  xEntropyEncodeMvCtu codes CTU `ctu`
 * of a width x height frame from its head mask and its 4 * popcount(head_mask) words of pack's form under `init` (NULL: the default):
 * it returns n_bytes, stores the first min(n_bytes, cap) bytes in out (which may be NULL with cap 0) and, with bins != NULL, the context
 * and the bypass bin counts; X266HIP_EINVAL for a malformed mask, a bad size, a ctu >= n_ctu, a NULL words, a NULL out with a cap or a
 * table entry outside 31 .. 2017.  xEntropyDecodeMvCtu writes the head mask, the payload (0, 0, low16(dx), low16(dy) per partition,
 * the rest of words[256] zero) and the number of partitions; it returns 0, or 1 for a malformed substream (then the flat CTU), or
 * X266HIP_EINVAL for a bad size, a ctu >= n_ctu, a NULL output, a NULL bytes with a length, an n_bytes above
 * X266_ENTROPY_MOTION_MAX_BYTES or a bad table. */
int xEntropyMvDefaultInit(uint16_t init[X266_ENTROPY_MOTION_CONTEXTS]);
int xEntropyEncodeMvCtu(int width, int height, size_t ctu, uint64_t head_mask, const uint16_t *words, const uint16_t *init, uint8_t *out,
                            size_t cap, uint32_t bins[2]);
int xEntropyDecodeMvCtu(int width, int height, size_t ctu, const uint8_t *bytes, size_t n_bytes, const uint16_t *init, uint64_t *head_mask,
                            uint16_t words[256], uint32_t *parts);

/* ---- the entropy coder of the side information: kinds, intra modes, coded flags, classes and qp as range-coded CTU substreams ----
 * The level substreams need the class bytes to be parsed, xQuantRegionsGpu(1) needs the qp, the deblocking calls need the kinds and
 * the intra reconstruction the modes; none of these is in the level or the motion stream.  xEntropyEncodeSideGpu codes what
 * xDct32CodeMixedFrameGpu, xTransformDecideCtuTilesGpu and xAqDecideGpu / xLaTreeQpGpu decide per 32x32 region into a third stream,
 * one independent substream per CTU under the range coder of the levels (above; the coder, its bytes, the stream's words and the
 * padding are exactly those); xEntropyDecodeSideGpu is its inverse.  With the level and the motion coder this holds everything the
 * chain needs to reconstruct a P-frame.  No upstream counterpart; the arithmetic here is the contract.
 *
 * Regions.  r = 6 ctu + q, q over Y0 Y1 Y2 Y3 U V, as the coding calls index them; Y0 Y1 are the top two luma regions of the CTU, Y2 Y3
 * the bottom two.  The calls take n_ctu, not a frame size: a region outside the frame still has its bytes.
 *
 * Canonical values: what is coded, and what decode returns.  Per CTU and q:
 *     K[q]   d_kind[r] != 0 for q <= 3.  There is ONE chroma kind: K[4] = K[5] = (d_kind[6 ctu + 4] != 0); entry 5 is ignored on
 *            encode, decode writes both entries.
 *     M[q]   for an intra region min(d_mode[r], 34), for an inter region 255.  There is one chroma mode, entry 4's: entry 5 is ignored on
 *            encode, decode writes it into entries 4 and 5.
 *     Z[q]   d_nnz[r] != 0: the region is CODED.  Decode writes 1 or 0.
 *     C[q]   k = d_class[r] & 15, and k = 3 when (k & 3) == 3: the transforms read a size-32 class of any type as the 32-point DCT-II,
 *            so C lies in X266_TDECIDE_CLASSES.  An uncoded region has C = 3.
 *     Q[q]   min(d_qp[r], 51).  An uncoded region has Q = its predictor (below).
 * A NULL array on encode: d_kind NULL = every kind 0; d_nnz NULL = every region coded; d_class NULL = every class 3; d_qp NULL = every
 * luma qp is `qp` and every chroma qp clamp(qp + chroma_qp_offset, 0, 51).  d_mode == NULL with d_kind != NULL is X266HIP_EINVAL.  A
 * NULL array on decode is not written.
 *
 * Syntax of a CTU.  For q = 0..3 in order: kind; the luma mode if intra; coded; if coded the class, then the qp difference.  Then the
 * chroma part: one kind; the chroma mode if intra; then for q = 4 and for q = 5: coded, and if coded the class, then the qp difference.
 * "Truncated unary of v with maximum m" is v one-bins and, if v < m, a zero-bin.
 *     kind          one bin, 1 = intra.  Contexts: luma, chroma.
 *     luma mode     HEVC's three most probable modes from A and B.  A is the mode of the left neighbour inside the CTU (q - 1 for odd
 *                   q), B of the above neighbour inside the CTU (q - 2 for q >= 2); a neighbour that is absent or inter counts as mode 1.
 *                   Nothing outside the CTU is read.  A == B < 2: {0, 1, 26}.  A == B >= 2: {A, 2 + ((A + 29) & 31), 2 + ((A - 1) & 31)}.
 *                   A != B: {A, B, the first of 0, 1, 26 that is neither}.  Bin mpm (one context), 1 = M is in the list.  If set: the
 *                   index as truncated unary with maximum 2 in bypass bins.  Otherwise the rank of M among the 32 other modes in
 *                   ascending order as 5 bypass bits, most significant first; every rank 0..31 names a mode.
 *     chroma mode   The list: M[0] if K[0], then 0, 26, 10, 1, duplicates dropped: 4 or 5 entries, in the order xDct32CodeMixedFrameGpu
 *                   tries them.  Bin listed (one context), 1 = M is in the list.  If set: the index as truncated unary with maximum
 *                   (entries - 1) in bypass bins.  Otherwise the rank among the 31 or 30 unlisted modes in ascending order as 5 bypass
 *                   bits; a decoded rank at or beyond their number is malformed.
 *     coded         one bin, Z.  Contexts: luma, chroma.
 *     class         bin small = (C != 3), contexts luma, chroma.  If set: 2 - (C & 3) as truncated unary with maximum 2, context per bin
 *                   (two), then C >> 2 as truncated unary with maximum 3, context per bin (three).
 *     qp difference d = Q - pred.  cur starts at `qp`.  A coded luma region has pred = cur and then sets cur = Q; an uncoded luma region
 *                   decodes to Q = cur.  U has pred = clamp(cur + chroma_qp_offset, 0, 51) with cur as Y3 left it; V has pred = U's Q,
 *                   coded or not.  Bins: nz (d != 0; contexts luma, chroma); gt1 (|d| > 1; one context); if set r = |d| - 2 <= 49 as
 *                   Exp-Golomb order 0 in bypass bins (v = r + 1, k = ilog2(v): k ones, a zero, the k low bits of v, most significant
 *                   first; k <= 5); the sign as a bypass bin, 1 = negative.  A prefix of more than 5 ones is malformed; a decoded Q
 *                   outside 0..51 is malformed.
 * Contexts.  X266_ENTROPY_SIDE_CONTEXTS = 16, in this order: kind luma, chroma; mpm; listed; coded luma, chroma; small luma, chroma; the
 * two bins of the size code; the three bins of the type code; nz luma, chroma; gt1.  They restart at every CTU from the call's table.
 * `init` is HOST memory, 16 uint16 in 31 .. 2017, read during the call and passed by value; NULL is the default table
 * (xEntropySideDefaultInit), all 1024: nothing measured justifies a skew.  The decoder must take the same table.
 *
 * Decoder rules.  Every loop is bounded: 6 regions, 5 list entries, 35 modes, unary codes of at most 2, 3 and 4 bins, 6 prefix bins, 5
 * suffix bits.  The malformed cases are the three above: a chroma rank beyond the unlisted modes, a qp prefix of more than 5 ones, a Q
 * outside 0..51.
 * The flat CTU: every kind 0 and no region coded.  Its 11 bins (5 kinds, 6 coded flags) are all zero bins, so it encodes to 0 bytes,
 * and zero bytes decode, under every table, to the flat CTU: kind 0, mode 255, d_nnz 0, class 3, qp equal to the predictors (`qp` for
 * luma, clamp(qp + chroma_qp_offset, 0, 51) for chroma).  This one rule covers every failure on decode: a record with offset >
 * cap_words, (n_bytes + 1) / 2 > cap_words - offset or n_bytes > X266_ENTROPY_SIDE_MAX_BYTES decodes as the flat CTU (d_status 1), and
 * so does a malformed substream (d_status 2).  Nothing outside [0, cap_words) of d_stream is ever read, and inside a substream only its
 * n_bytes count.
 * Round trip.  Decode of encode returns the canonical form of the input, exactly, for every input byte value; encode of that canonical
 * form gives the same bytes.
 *
 * The largest substream.  Context bins: a luma region has kind, mpm, coded, small, 2 + 3 class bins, nz, gt1 = 11, the chroma part kind
 * and listed and per region coded, small, 2 + 3, nz, gt1 = 2 + 2 x 9: 64 in all, each under 6.05 bits (the level coder's bound).  Bypass
 * bins: a mode rank is 5 (an index is at most 4), a qp difference at most 5 + 1 + 5 + 1 = 12: 4 x 17 + 5 + 2 x 12 = 97, each under
 * 1.0001 bits.  That is under 485 bits, no more than 61 byte shifts, and with the termination 65 bytes: X266_ENTROPY_SIDE_MAX_BYTES =
 * 80, a multiple of 16.  (The worst CTU that can be built -- every region intra with an unlisted mode, every class 12, every
 * difference +-51 -- comes to 20 bytes under the default table and to 43 under a table of 2017s; the bound is the floor's, not a
 * measured one.)
 *
 * Worked values, qp 32 and chroma_qp_offset 0 unless said, under the default table, bytes in hex (context bins, bypass bins):
 *     the flat CTU:                                                        no bytes (11, 0)
 *     Y0 intra with mode 26 (list {0, 1, 26}, index 2), nothing coded:     f0 (12, 2)
 *     Y0 intra with mode 10 (rank 8 of the 32 others), nothing coded:      8f ff fc (12, 5)
 *     chroma intra with mode 34 (list {0, 26, 10, 1}, rank 30):            01 0c 0e (12, 5)
 *     Y0 coded with class 0, Y1 coded with class 14, both d = 0:           78 df ae (22, 0)
 *     Y0 coded with Q = 33 (d = +1):                                       50 (14, 1)
 *     qp 51, Y0 coded with Q = 0 (d = -51):                                5f d2 7c (14, 12)
 *     every array NULL (all inter, all coded, class 3, d = 0):             44 4d 5a (23, 0)
 *
 * xEntropyEncodeSideGpu writes every record of d_coded.  offset there is the exclusive prefix sum of n_words, in 64 bits; d_total[0] =
 * the total number of words, d_total[1] = the number of leading CTUs whose substream lies completely inside cap_words.  A substream is
 * written if and only if offset + n_words <= cap_words; no word at or beyond cap_words is ever written.  cap_words == 0 with d_stream
 * == NULL is the count-only call.  n_ctu == 0 writes d_total = {0, 0} and nothing else.  Three launches on the caller's stream: count
 * and records, the offsets (the scan of xLevelsPackGpu), write.
 * xEntropyDecodeSideGpu trusts nothing in a record of d_coded but offset and n_bytes, and holds both against cap_words before any load.
 * It writes the six entries of every output array that is not NULL, and d_status, if not NULL: 0 (good), 1 (record outside the
 * capacity) or 2 (malformed substream) per CTU.  d_total is ignored; d_stream may be NULL when cap_words == 0.  One launch; n_ctu == 0
 * launches nothing.
 * Both: ONE LANE per CTU -- a CTU has at most 161 bins, too few to give it a wave --, the coder's state in the lane's registers, its 16
 * contexts and its bytes in LDS; no atomics, no allocation; the same input gives the same bytes on every run and under every launch
 * option; the calls can be captured into a graph.
 *
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned required buffer (d_coded,
 * d_stream unless cap_words == 0, d_total on encode; alignments: the field comments), d_kind without d_mode on encode, an entry of init
 * outside 31 .. 2017, qp outside 0..51, chroma_qp_offset outside -12..12, a span that does not fit in the address space, an output
 * overlapping any other buffer.  The extents are 6 bytes per CTU for d_kind, d_mode, d_class and d_qp, 24 for d_nnz, 32 for d_coded,
 * cap_words * 2 for d_stream, 16 for d_total, one byte per CTU for d_status.  With n_ctu == 0 only the scalars, init and d_total of
 * the encode call are looked at.
 * Out of scope: direction bytes of B-frames; SAO and ALF parameters; a frame header or any container around the three streams; context
 * carry-over between CTUs; deriving class_bits of the transform decision from a table.  (No longer out of scope: adapted tables, a
 * frame's own through xEntropyStatsSideGpu and xEntropyInitFromCounts, below.) */
#define X266_ENTROPY_SIDE_CONTEXTS  16
#define X266_ENTROPY_SIDE_MAX_BYTES 80
typedef struct x266_entropy_side_ctu_t {   /* 32 bytes; the first 20 bytes are laid out as x266_level_region_t's */
    uint32_t ctx_bins;     /* context-coded bins of the CTU                                      */
    uint32_t bypass_bins;  /* bypass bins of the CTU                                             */
    uint64_t offset;       /* start of the CTU's substream in d_stream, in 16-bit words          */
    uint32_t n_words;      /* (n_bytes + 1) / 2                                                  */
    uint32_t n_bytes;      /* bytes of the substream, 0 .. X266_ENTROPY_SIDE_MAX_BYTES           */
    uint32_t n_intra;      /* intra regions of the CTU, 0 .. 6 (V counts with U's kind)          */
    uint32_t n_coded;      /* coded regions of the CTU, 0 .. 6                                   */
} x266_entropy_side_ctu_t;
typedef struct x266_entropy_side_t {
    uint8_t  *d_kind;                  /* [6 n_ctu] or NULL, any alignment; encode reads, decode writes                        */
    uint8_t  *d_mode;                  /* [6 n_ctu] or NULL, any alignment; encode reads, decode writes                        */
    uint8_t  *d_class;                 /* [6 n_ctu] or NULL, any alignment; encode reads, decode writes                        */
    uint8_t  *d_qp;                    /* [6 n_ctu] or NULL, any alignment; encode reads, decode writes                        */
    uint32_t *d_nnz;                   /* [6 n_ctu] or NULL, 4-byte aligned; encode reads, decode writes (1 or 0)               */
    x266_entropy_side_ctu_t *d_coded;  /* [n_ctu], 8-byte aligned; encode writes, decode reads offset and n_bytes only         */
    uint16_t *d_stream;                /* [cap_words], 16-byte aligned; the coded bytes, little-endian words as the level coder's */
    uint64_t *d_total;                 /* [2], 8-byte aligned; encode writes {words, leading CTUs that fit}; decode ignores (may be NULL there) */
    uint8_t  *d_status;                /* [n_ctu] or NULL, any alignment; decode only: 0 good, 1 record outside the capacity, 2 malformed substream */
    const uint16_t *init;              /* HOST memory, [X266_ENTROPY_SIDE_CONTEXTS], or NULL: the default table                */
    size_t    n_ctu;
    uint64_t  cap_words;
    int       qp;                      /* 0..51, the frame's                                                                   */
    int       chroma_qp_offset;        /* -12..12                                                                              */
} x266_entropy_side_t;
int xEntropyEncodeSideGpu(x266hip_ctx *ctx, const x266_entropy_side_t *p, void *stream);
int xEntropyDecodeSideGpu(x266hip_ctx *ctx, const x266_entropy_side_t *p, void *stream);
/* Host only, the functions the kernels run.  xEntropySideDefaultInit writes the default table.  xEntropyEncodeSideCtu codes one CTU from
 * six entries of each array (a NULL array as on the device call) under `init` (NULL: the default): it returns n_bytes, stores the first
 * min(n_bytes, cap) bytes in out (which may be NULL with cap 0) and, with bins != NULL, the context and the bypass bin counts;
 * X266HIP_EINVAL for kind without mode, a NULL out with a cap, a qp or chroma_qp_offset out of range or a table entry outside 31 .. 2017.
 * xEntropyDecodeSideCtu writes six entries of every array that is not NULL; it returns 0, or 1 for a malformed substream (then the flat
 * CTU), or X266HIP_EINVAL for a NULL bytes with a length, an n_bytes above X266_ENTROPY_SIDE_MAX_BYTES, a bad scalar or a bad table. */
int xEntropySideDefaultInit(uint16_t init[X266_ENTROPY_SIDE_CONTEXTS]);
int xEntropyEncodeSideCtu(const uint8_t *kind, const uint8_t *mode, const uint8_t *cls, const uint8_t *qp_in, const uint32_t *nnz, int qp,
                          int chroma_qp_offset, const uint16_t *init, uint8_t *out, size_t cap, uint32_t bins[2]);
int xEntropyDecodeSideCtu(const uint8_t *bytes, size_t n_bytes, int qp, int chroma_qp_offset, const uint16_t *init, uint8_t *kind, uint8_t *mode,
                          uint8_t *cls, uint8_t *qp_out, uint32_t *nnz);

/* ---- per-context bin statistics on the device, and initial tables from them ----
 * The level and the side coder start every substream from a static table.  These calls count, per context, the zero and the one bins
 * that a frame's arrays put into that context, and turn the counts into an initial table.  Which context a bin goes to and whether it is
 * 0 or 1 depends on the coded arrays alone -- not on the table, the coder's state or the order of the bins -- so the counts need no
 * coder.  The calls read exactly what the encoders read, which is exactly what the decoders write: a decoder that runs them on frame
 * N's decoded arrays derives the table the encoder derived from the same arrays, and both code frame N + 1 under it.  Backward
 * adaptation per frame: no table crosses the wire and every substream stays independent.
 *
 * Counts.  An array of 2 * n_contexts counters: counts[2 c] the zero bins of context c, counts[2 c + 1] its one bins, c in the order of
 * the coder's table (X266_ENTROPY_CONTEXTS = 100 for levels, size 4 first; X266_ENTROPY_SIDE_CONTEXTS = 16 for side information).
 * Bypass bins are not counted.
 *
 * xEntropyInitFromCounts: for context c with z = counts[2 c], o = counts[2 c + 1] and n = z + o, in unsigned 64-bit integers,
 *     n == 0:    init[c] = 1024
 *     otherwise: init[c] = (4096 z + n) / (2 n)   (integer division: 2048 z / n rounded half up), then held to 31 .. 2017.
 * It returns 0, or X266HIP_EINVAL -- nothing written -- for a NULL counts or init with n_contexts != 0 or any z or o of 2^51 or more
 * (4096 z + n stays below 2^64).  n_contexts is the caller's: 100, 16 or any other.
 *
 * xEntropyCountRegion ADDS to counts[200] the context bins of one region: the walk of the level coder's syntax (above) over the 1024
 * levels under class `cls` (only cls & 3 counts) with a sink that counts instead of coding -- the one copy of the syntax, not a second.
 * coded == 0 is the encoder's d_nnz[r] == 0 case: the region's 64 >> 2 k blocks (k = cls & 3) each give one zero cbf bin of size k and
 * level is not read (it may be NULL).  X266HIP_EINVAL for a NULL counts, or a NULL level with coded != 0.
 * xEntropyCountSideCtu ADDS to counts[32] the context bins of one CTU from six entries of each array, with the NULL conventions and the
 * canonical form of xEntropyEncodeSideCtu; X266HIP_EINVAL for kind without mode, a NULL counts, a qp or chroma_qp_offset out of range.
 * For both, the sum of what a call adds equals bins[0] of the matching encode helper under any table.  These two are the definition
 * the device calls are held against.
 *
 * xEntropyStatsLevelsGpu reads d_level, d_class (or NULL: every region 32x32) and d_nnz (or NULL) exactly as xEntropyEncodeLevelsGpu
 * does, a region with d_nnz[r] == 0 counting as all zero with its levels not read, and writes
 *     d_counts   uint64[2 * X266_ENTROPY_CONTEXTS]: the sum of xEntropyCountRegion over the n_regions regions, for every input.  Hence
 *                the sum over d_counts equals the sum of ctx_bins over the records of xEntropyEncodeLevelsGpu on the same arrays.
 *     d_part     uint32[xEntropyStatsRows(n_regions, X266_ENTROPY_STATS_REGIONS)][2 * X266_ENTROPY_CONTEXTS]: row j holds the counts of
 *                the regions [j * X266_ENTROPY_STATS_REGIONS, (j + 1) * X266_ENTROPY_STATS_REGIONS) that exist.  It is contract, not
 *                scratch: a host forms per-slice tables from its rows.  A region has at most 3456 context bins, a row at most
 *                32 * 3456 = 110 592: no counter of a row can pass 32 bits.
 * xEntropyStatsSideGpu reads the five arrays, qp and chroma_qp_offset as xEntropyEncodeSideGpu does (same NULL conventions, the
 * canonical form is what is counted, so the counts of any arrays equal the counts of their decoded form) and writes d_counts
 * uint64[2 * X266_ENTROPY_SIDE_CONTEXTS], the sum of xEntropyCountSideCtu over the n_ctu CTUs, and d_part
 * uint32[xEntropyStatsRows(n_ctu, X266_ENTROPY_SIDE_STATS_CTUS)][2 * X266_ENTROPY_SIDE_CONTEXTS], row j the CTUs [64 j, 64 j + 64); a
 * CTU has at most 64 context bins (11 for each of Y0..Y3 and U, 9 for V).
 * xEntropyStatsRows(n_units, per_row) = ceil(n_units / per_row), 0 for per_row == 0.
 * Both calls: two launches on the caller's stream -- the rows, then one workgroup that adds the rows in ascending order --, no global
 * atomics, no allocation, no host synchronisation; they can be captured into a graph; the same input gives the same bytes on every run.
 * They read no launch option.  n == 0 writes the zeros of d_counts and nothing else (d_part and the inputs are not looked at).
 * The level kernel is a data-parallel statement of the syntax, not the coder's serial walk: one wave per region at a time, lane g = CG
 * bit g, the scan-ordered significance, |l| > 1 and |l| > 2 maps of its 16 levels, and every count from ballots and popcounts.  The side
 * kernel takes one lane per CTU and runs the syntax's own walk with the counting sink.
 *
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p, a NULL or misaligned d_counts (8 bytes), and
 * with n != 0 a NULL or misaligned d_part (16), d_level (16) or d_nnz (4, if given), d_kind without d_mode, qp outside 0..51 or
 * chroma_qp_offset outside -12..12 (side call, also with n == 0), a span that does not fit in the address space, an output overlapping
 * any other buffer.  Extents: d_counts 1600 (levels) or 256 (side) bytes, d_part rows * 800 or rows * 128 bytes, the inputs as on the
 * encode calls.
 * Left out on purpose, a follow-up if it ever pays: the motion coder.  Its contexts number 7, its stream is 3 473 of the measured frame's
 * 424 933 bytes, and 1 947 of 2 040 CTUs cost no byte.  Neither call changes a default table. */
#define X266_ENTROPY_STATS_REGIONS   32
#define X266_ENTROPY_SIDE_STATS_CTUS 64
typedef struct x266_entropy_stats_t {
    const int16_t  *d_level;           /* [n_regions * 1024], 16-byte aligned                                          */
    const uint8_t  *d_class;           /* [n_regions] or NULL (every region 32x32), any alignment                      */
    const uint32_t *d_nnz;             /* [n_regions] or NULL, 4-byte aligned                                          */
    uint64_t *d_counts;                /* [2 * X266_ENTROPY_CONTEXTS], 8-byte aligned                                  */
    uint32_t *d_part;                  /* [rows][2 * X266_ENTROPY_CONTEXTS], 16-byte aligned                           */
    size_t    n_regions;
} x266_entropy_stats_t;
typedef struct x266_entropy_side_stats_t {
    const uint8_t  *d_kind;            /* [6 n_ctu] or NULL, any alignment                                             */
    const uint8_t  *d_mode;            /* [6 n_ctu] or NULL, any alignment                                             */
    const uint8_t  *d_class;           /* [6 n_ctu] or NULL, any alignment                                             */
    const uint8_t  *d_qp;              /* [6 n_ctu] or NULL, any alignment                                             */
    const uint32_t *d_nnz;             /* [6 n_ctu] or NULL, 4-byte aligned                                            */
    uint64_t *d_counts;                /* [2 * X266_ENTROPY_SIDE_CONTEXTS], 8-byte aligned                             */
    uint32_t *d_part;                  /* [rows][2 * X266_ENTROPY_SIDE_CONTEXTS], 16-byte aligned                      */
    size_t    n_ctu;
    int       qp;                      /* 0..51, the frame's                                                           */
    int       chroma_qp_offset;        /* -12..12                                                                      */
} x266_entropy_side_stats_t;
int xEntropyStatsLevelsGpu(x266hip_ctx *ctx, const x266_entropy_stats_t *p, void *stream);
int xEntropyStatsSideGpu(x266hip_ctx *ctx, const x266_entropy_side_stats_t *p, void *stream);
size_t xEntropyStatsRows(size_t n_units, size_t per_row);
int xEntropyInitFromCounts(const uint64_t *counts, size_t n_contexts, uint16_t *init);
int xEntropyCountRegion(const int16_t *level, int cls, int coded, uint64_t counts[2 * X266_ENTROPY_CONTEXTS]);
int xEntropyCountSideCtu(const uint8_t *kind, const uint8_t *mode, const uint8_t *cls, const uint8_t *qp_in, const uint32_t *nnz, int qp,
                         int chroma_qp_offset, uint64_t counts[2 * X266_ENTROPY_SIDE_CONTEXTS]);

/* ---- frame quality: SSE, PSNR and SSIM of a decoded tiled frame against its source, per CTU and per frame ----
 * The instrument behind every statement about RDOQ, the transform decision and the loop filters: the distortion between a source
 * frame and a decoded frame, for luma and both chroma planes, computed where the frames live and reduced to 48 bytes per CTU and
 * 64 bytes per frame.  No upstream counterpart: the SSIM is x264's (its ssim_end1 over 8x8 windows on a grid of 4x4 blocks), as
 * recalled, in integers; the arithmetic here is the contract.
 *
 * Geometry.  Frame sides are positive multiples of 16; tiles are 16x16 in raster order, width / 16 per row; CTUs are
 * ceil(width / 64) x ceil(height / 64) in raster order.  A tile's luma is m_Y, its chroma m_C: 8 rows of 8 interleaved (U, V)
 * pairs; m_I is never read.  a is a sample of d_src, b the co-located sample of d_dec.
 *
 * SSE, per plane and CTU: the sum of (a - b)^2 over the CTU's in-frame samples, at most 4096 * 65025, which fits uint32.
 *
 * SSIM, per plane on the plane's grid of 4x4 blocks: W4 = width / 4 by H4 = height / 4 blocks for luma; a chroma plane is
 * (width / 2) x (height / 2) samples, its grid width / 8 by height / 8 blocks.  A window sits at every block position (bx, by) with
 * 0 <= bx < W4 - 1 and 0 <= by < H4 - 1 (the plane's own W4, H4) and covers the 8x8 samples of blocks (bx .. bx + 1, by .. by + 1);
 * it belongs to the CTU of its top-left block, (bx >> 4, by >> 4) for luma and (bx >> 3, by >> 3) for chroma.  Windows cross tile
 * and CTU borders freely.  A 16x16 frame has 9 luma windows and 1 window per chroma plane.
 * Per window, over its 64 samples: S1 = sum a, S2 = sum b, SS = sum (a^2 + b^2), S12 = sum a b, and
 *   vars  = 64 SS - S1^2 - S2^2            covar = 64 S12 - S1 S2   (signed)
 *   ln    = 2 S1 S2 + 416                  ld    = S1^2 + S2^2 + 416
 *   cn    = 2 covar + 235963  (signed)     cd    = vars + 235963
 *   lq    = (ln << 30) / ld                                  unsigned 64-bit
 *   cq    = sign(cn) * ((|cn| << 30) / cd)                   the quotient truncates toward zero, as C's / does
 *   q     = (lq * cq) >> 30                                  an arithmetic shift of the signed 64-bit product: it floors
 * 416 and 235963 are x264's ssim_c1 and ssim_c2 for 8-bit samples.  Always ln <= ld and |cn| <= cd, so |q| <= 2^30, and no
 * intermediate passes 2^61.  Identical windows give exactly 2^30; all 0 against all 255 gives 1677; an 8x8 checkerboard of 0 / 255
 * ((x + y) & 1) against its inverse gives cn = -132935237 and q = -1069943477.
 * ssim[p] of a CTU's record is the sum of q over the CTU's windows of plane p (Y, U, V), win_y and win_c their counts (the two
 * chroma planes have the same windows).  With a flag off, that flag's fields are written 0.
 * d_total[8]: sse Y, U, V, then ssim Y, U, V, then win_y, then win_c, each summed over all CTUs.
 *
 * xQualityStatsGpu takes one host struct, read during the call and never from the device; the pointers in it are device pointers
 * (alignments: the field comments).  It reads d_src and d_dec and writes every record of d_ctu, those of partial CTUs included; then,
 * if d_total is given, a second launch of ONE workgroup adds the records xQualityTotalsChunk() at a time -- integer sums, no
 * atomics, the same bytes on every run.  The call allocates nothing, does not synchronise, launches on the caller's stream, can be
 * captured into a graph, and its result does not depend on any launch option.  It sits after reconstruction or after the last loop
 * filter of a frame, on the frame the next one will predict from.
 * X266HIP_EINVAL, with nothing launched and the call named in xHipLastError: a NULL p; a NULL or misaligned d_src, d_dec or d_ctu; a
 * misaligned d_total; a side that is not a positive multiple of 16; flags that are 0 or have other bits set; a span that does not
 * fit in the address space; an output overlapping any other buffer of the call (the two inputs may coincide).  The extents are
 * width * height * 2 (d_src, d_dec), 48 n_ctu (d_ctu) and 64 bytes (d_total). */
#define X266_QUALITY_SSE  1
#define X266_QUALITY_SSIM 2
typedef struct x266_quality_ctu_t {
    int64_t  ssim[3];      /* Y, U, V: sum of the windows' Q30 values                                       */
    uint32_t sse[3];       /* Y, U, V: sum of (src - dec)^2 over the CTU's in-frame samples                 */
    uint32_t win_y, win_c; /* windows counted into ssim[0], and into each of ssim[1], ssim[2]               */
    uint32_t reserved;     /* written 0                                                                     */
} x266_quality_ctu_t;      /* 48 bytes */
typedef struct x266_quality_t {
    const x266_ref_block_t *d_src;   /* [n_tiles], 16-byte aligned                                          */
    const x266_ref_block_t *d_dec;   /* [n_tiles], 16-byte aligned; may equal d_src                         */
    x266_quality_ctu_t *d_ctu;       /* [n_ctu], 16-byte aligned; output                                    */
    int64_t *d_total;                /* [8] or NULL, 8-byte aligned; output                                 */
    int width, height;               /* positive multiples of 16                                            */
    int flags;                       /* X266_QUALITY_SSE | X266_QUALITY_SSIM, not 0                         */
} x266_quality_t;
int xQualityStatsGpu(x266hip_ctx *ctx, const x266_quality_t *p, void *stream);
/* Records the totals' workgroup of xQualityStatsGpu takes per step (a test walks CTU counts around it). */
int xQualityTotalsChunk(void);
/* PSNR and SSIM from a frame's totals (host only; reads 8 int64, host memory; plain IEEE double throughout).  For p of Y, U, V:
 * psnr[p] = 10 log10(65025 N_p / sse_p) with N = width * height for Y and a quarter of it for each chroma plane; psnr[3] is the same
 * over the three planes' summed SSE and summed samples; 100.0 exactly where the SSE is 0.  ssim[p] = total / (win_p * 2^30), or 1.0
 * where the plane has no window.  X266HIP_EINVAL: a NULL pointer, a side that is not a positive multiple of 16, a negative SSE, or
 * window counts that are not the geometry's -- each either 0 (a run without X266_QUALITY_SSIM) or (W4 - 1) * (H4 - 1) of its plane. */
int xQualityFromTotals(const int64_t total[8], int width, int height, double psnr[4], double ssim[3]);

/* Synthetic residual stream with the reference's stimulus distribution
 * ((rand()&0xFF)-(rand()&0xFF), src_tb/dct32.c:191-193) from a counter-based
 * SplitMix64: sample i = lo8(r) - lo8(r>>8), r = mix(seed+(first_index+i+1)*phi). */
/* Alignment in bytes: d_dst 16. */
int xFillResidualDev(x266hip_ctx *ctx, int16_t *d_dst, size_t n_samples,
                     uint64_t seed, uint64_t first_index, void *stream);

/* ------------------------------------------------------------------------ */
/* batch API, host pointers (caller-owned host buffers; staged through        */
/* internal device buffers in chunks, H2D / kernel / D2H overlapped).         */
/* Synchronous: results are in `out` on return.                               */
/* ------------------------------------------------------------------------ */
/* Rates over a PCIe 5.0 x16 link that gives 57 GB/s one way and 48.5 GB/s each way when both directions run: 43 GB/s each way
 * from PINNED host buffers (xHipHostAlloc below, hipHostMalloc, or memory the host registered), 27 GB/s each way from pageable ones
 * -- the runtime stages pageable copies through the calling thread, so uploads and downloads take turns
 * (profiles/r04_hostpipe.txt).  A host that re-uses its buffers should allocate them pinned. */
int xDct32FwdBatch(x266hip_ctx *ctx, const int16_t *in, int16_t *out, size_t n_blocks);
int xDct32InvBatch(x266hip_ctx *ctx, const int16_t *in, int16_t *out, size_t n_blocks);
int xSatd8x8Batch(x266hip_ctx *ctx, const int16_t *diff, uint32_t *out, size_t n_blocks);

/* ------------------------------------------------------------------------ */
/* device memory / stream helpers for hosts without HIP headers               */
/* ------------------------------------------------------------------------ */
int xHipMalloc(x266hip_ctx *ctx, void **d_ptr, size_t bytes);
/* Page-locked host memory (hipHostMalloc) for the host-pointer batch calls and xHipMemcpy*: copies from / to it are true DMA. */
int xHipHostAlloc(x266hip_ctx *ctx, void **h_ptr, size_t bytes);
int xHipHostFree(x266hip_ctx *ctx, void *h_ptr);
int xHipFree(x266hip_ctx *ctx, void *d_ptr);
int xHipMemcpyH2D(x266hip_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int xHipMemcpyD2H(x266hip_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int xHipStreamSync(x266hip_ctx *ctx, void *stream);
int xHipStreamCreate(x266hip_ctx *ctx, void **stream);     /* a non-blocking hipStream_t */
int xHipStreamDestroy(x266hip_ctx *ctx, void *stream);
/* HIP graphs for launch-bound sequences (a frame's handful of small kernels costs more in launch
 * overhead than in execution): everything enqueued on `stream` (not the NULL stream) between
 * xHipGraphBegin and xHipGraphEnd -- any of the ...Dev calls above, in any number -- is recorded
 * instead of run, and xHipGraphLaunch replays the whole sequence with one submission.  The recorded
 * calls keep their pointer and size arguments, so a graph is replayed over the same buffers with new
 * contents.  xSatd8x8SearchDev and xSatd8x8SearchFromTilesDev size an internal scratch buffer per (stream, frame size) on first
 * use, which is illegal inside a capture: call xHipMeScratchReserve (below) or run one search on that stream beforehand. */
typedef struct x266hip_graph x266hip_graph;
int xHipGraphBegin(x266hip_ctx *ctx, void *stream);
int xHipGraphEnd(x266hip_ctx *ctx, void *stream, x266hip_graph **graph);
int xHipGraphLaunch(x266hip_ctx *ctx, x266hip_graph *graph, void *stream);
void xHipGraphFree(x266hip_ctx *ctx, x266hip_graph *graph);
/* Times `reps` back-to-back launches of one kernel with HIP events recorded on
 * `stream` itself; returns the mean milliseconds per launch in *ms_per_launch.
 * op: 0 = dct32 fwd, 1 = dct32 inv, 2 = satd8x8 (buffers as in the Dev calls); 3 .. 6 = xHipMemCeilingDev copy / read /
 * write / read probe of n_blocks * 2048 bytes. */
int xHipTimeKernel(x266hip_ctx *ctx, int op, const void *d_in, void *d_out,
                   size_t n_blocks, int reps, void *stream, double *ms_per_launch);
/* What THIS box's memory system gives the launch shape of the streaming kernels, with no arithmetic -- so that a report can
 * put "fraction of this box's copy / read rate" next to "fraction of the 8 TB/s spec" (boxes differ by 3-10 %).
 * kind X266_MEM_COPY: d_dst[0 .. bytes) = d_src[0 .. bytes) (16 bytes per lane, nontemporal 1 KiB-linear loads, "sc1 nt"
 * stores: the access pattern of the DCT / transform kernels); X266_MEM_READ: the same loads and nothing written but one
 * 32-bit XOR of the words of every 2 KiB piece, d_dst[piece] as uint32 (so d_dst holds 4 * ceil(bytes / 2048) bytes: the
 * pattern of the SATD / SAD kernels; the checksums make the stream checkable); X266_MEM_WRITE: nothing read (d_src may be
 * NULL), every 16-byte chunk c of d_dst = {(uint32)c, 0, 0, 0} with the same stores (the pattern of the intra predictor).
 * X266_MEM_READ_PROBE: X266_MEM_READ that stores a piece's XOR only where it equals X266_MEM_PROBE_MAGIC, i.e. practically
 * never: the rate of loads with nothing flowing back (a host that wants to see the loads happen plants a piece with that XOR).
 * bytes a multiple of 16, buffers 16-byte aligned.
 * Asynchronous on `stream`; time it with the event calls below or xHipTimeKernel's ops 3 / 4 / 5 / 6. */
#define X266_MEM_COPY 0
#define X266_MEM_READ 1
#define X266_MEM_WRITE 2
#define X266_MEM_READ_PROBE 3
#define X266_MEM_PROBE_MAGIC 0x12345678u
/* Alignment in bytes: d_src 16, d_dst 16. */
int xHipMemCeilingDev(x266hip_ctx *ctx, int kind, const void *d_src, void *d_dst, size_t bytes, void *stream);
/* HIP events for hosts without HIP headers, so that ANY sequence of the ...Dev calls can be timed on the
 * stream it is launched on (record an event before every launch and one after the last: consecutive
 * differences are per-launch durations).  xHipEventElapsedMs waits for `stop` and returns stop - start. */
int xHipEventCreate(x266hip_ctx *ctx, void **event);
int xHipEventDestroy(x266hip_ctx *ctx, void *event);
int xHipEventRecord(x266hip_ctx *ctx, void *event, void *stream);
int xHipEventElapsedMs(x266hip_ctx *ctx, void *start, void *stop, double *ms);

/* ------------------------------------------------------------------------ */
/* one node, several GPUs (BASELINE configs[4])                    */
/*                                                                          */
/* Blocks are independent (src_tb/dct32.c:75,167-168; satd8x8 is a pure      */
/* function, src_tb/satd.c:31-118), so the only multi-GPU traffic is moving   */
/* shards: the root rank (rank 0) owns the frame, every rank gets a           */
/* contiguous shard of each batch, transforms it, and returns the results.    */
/* Transport is RCCL point-to-point: ONE ncclGroupStart/End of               */
/* ncclSend/ncclRecv per step, so that all of the root's xGMI links and both  */
/* directions of each are busy at once; librccl.so.1 is opened on first use   */
/* (dlopen), so hosts that never create a node do not load it; a process that   */
/* has already loaded an RCCL (e.g. torch's bundled one) shares that copy.  The  */
/* environment variable X266HIP_RCCL_LIB, when set, names the library to open   */
/* INSTEAD (another RCCL build; the repository's tests point it at their        */
/* single-box model of RCCL's semantics) -- xHipNodeRcclInfo tells which        */
/* library and version a process ended up with.  A failed communication step    */
/* aborts the node's communicators (ncclCommAbort) so that no rank is left in a */
/* group that cannot complete; the node is then good for xHipNodeFree only and   */
/* every rank must treat the failure the same way.  Two process                  */
/* models, same calls afterwards:                                             */
/*   xHipNodeInit      one process drives n devices (ncclCommInitAll)         */
/*   xHipNodeInitRank  one process per GPU (ncclCommInitRank); every rank     */
/*                     makes the same sequence of xNode... calls              */
/* ------------------------------------------------------------------------ */
#define X266HIP_ECOMM    (-4)   /* RCCL unavailable or a communication call failed */
#define X266HIP_NODE_ID_BYTES 128
typedef struct x266hip_node x266hip_node;
typedef struct x266hip_nstream x266hip_nstream;

/* Host-only planning (no device needed; also what the CPU tests of the N > 1 logic call).
 * xShardRange: rank's contiguous [begin, end) of n_units; the first n_units % world ranks take one extra.
 * xMeStripePlan: motion search partition into horizontal stripes of 8-pixel block rows -- stripe's block
 * rows [*block_row_begin, *block_row_end) and the reference rows [*ref_row_begin, *ref_row_end) it reads
 * (frame row coordinates of the padded reference: may be negative / exceed height by up to `range`; the
 * halo is read-only input that travels with the scatter, there is no exchange step).  Returns 0 / EINVAL. */
int  xShardRange(size_t n_units, int rank, int world, size_t *begin, size_t *end);
int  xMeStripePlan(int height, int range, int stripe, int n_stripes, int *block_row_begin, int *block_row_end,
                   int *ref_row_begin, int *ref_row_end);

int  xHipNodeInit(x266hip_node **node, const int *devices, int n_devices);       /* devices NULL: 0..n-1 */
int  xHipNodeUniqueId(void *id /* X266HIP_NODE_ID_BYTES, from rank 0, handed to every rank by the host */);
int  xHipNodeInitRank(x266hip_node **node, int device, int rank, int world, const void *id);
void xHipNodeFree(x266hip_node *node);
int  xHipNodeWorld(const x266hip_node *node);
int  xHipNodeLocalCount(const x266hip_node *node);                               /* ranks driven by this process */
int  xHipNodeLocalRank(const x266hip_node *node, int local_index);               /* their global ranks */
x266hip_ctx *xHipNodeCtx(x266hip_node *node, int local_index);                   /* owned by the node */
const char *xHipNodeLastError(const x266hip_node *node);
/* "transport": 0 RCCL send/recv groups (default), 1 hipMemcpyPeerAsync (single-process nodes only);
 * "me_local_copy": 1 = the root's own motion-search stripes also go through stripe buffers (what a peer
 * receives) instead of being searched in place -- exercises the halo logic on one GPU (default 0). */
int  xHipNodeSetOption(x266hip_node *node, const char *key, int value);
/* Communication self-check: every rank sends a pattern to the next rank and receives from the previous
 * one inside one RCCL group (with one rank: to itself), then all ranks all-reduce a checksum. */
int  xHipNodeSelfTest(x266hip_node *node);
/* The RCCL this process uses: NCCL_VERSION_CODE-style version (0 if the library has no ncclGetVersion) and the path of
 * the shared object (dladdr).  X266HIP_ECOMM when no RCCL could be opened. */
int  xHipNodeRcclInfo(int *version, char *path, size_t path_cap);

/* A stream of frames, each a fixed set of "lanes" (one batch per lane).  op: 0 = DCT32 forward
 * (2048 B in / 2048 B out per unit), 1 = DCT32 inverse, 2 = 8x8 SATD (128 B in / 4 B out).
 * xNodeFrameStreamCreate: the two lanes of BASELINE configs[4] for a width x height luma frame:
 * (width/32)*(height/32) DCT32 blocks and (width/8)*(height/8) SATD blocks. */
int  xNodeStreamCreate(x266hip_node *node, int n_lanes, const int *ops, const size_t *max_units, x266hip_nstream **s);
int  xNodeFrameStreamCreate(x266hip_node *node, int width, int height, x266hip_nstream **s);
void xNodeStreamFree(x266hip_nstream *s);
/* Step t (the t-th Push/Flush step of this stream), pipelined and asynchronous: one RCCL group moves
 * frame t's shards root -> peers AND frame t-2's results peers -> root, then every rank's kernels for
 * frame t are enqueued; so while frame t is transformed, frame t+1's inputs and frame t-1's outputs
 * are on the links.  d_in[lane] / d_out[lane]: on the process that drives the root rank, device
 * pointers on the root's device of the lane's input units and of the caller-owned buffer that receives
 * its results (zero-copy: the root transforms its own shard in place, peers' shards are sent from /
 * received into these buffers directly); ignored on other processes (may be NULL).  units[lane]
 * (NULL: the stream's max_units) must be the same on every rank.  producer_stream: the root-device
 * stream the inputs were produced on (ordering by event; NULL = the default stream).
 * A step's ticket may be waited for once TWO later steps have been issued (Push or Flush); its inputs may be
 * overwritten once THREE later steps have been issued (or its ticket has been waited for): until then its buffers belong
 * to the stream -- the kernels of three consecutive frames run on three streams and may overlap (only a third frame in
 * flight covers the ramp and tail of ~30 us kernels), so frames t, t+1 and t+2 must not share buffers: input rings of four,
 * output rings of five or more (X266_STREAM_IN_RING / X266_STREAM_OUT_RING; they grew by one when the stream went from two to three
 * frames in flight, so a host sizes its rings by the constants, not by a number).  Input buffers may be SHARED between frames (they
 * are only read); an output buffer that overlaps the output of one of the previous X266_STREAM_OUT_RING - 1 frames of this stream
 * -- frames not yet flushed -- is refused with X266HIP_EINVAL: two frames in flight would write it.  *ticket (may be NULL) receives t. 
 * One process per GPU (xHipNodeInitRank): a push is a collective step.  A call that fails on ONE rank -- including an argument
 * error only the root can detect (its buffers) -- leaves the other ranks' step unmatched; the failing rank's node is marked
 * failed (every later call returns X266HIP_ECOMM) and the host must free the node on every rank, as after any ECOMM. */
#define X266_STREAM_IN_RING  4
#define X266_STREAM_OUT_RING 5
int  xNodeStreamPush(x266hip_nstream *s, const void *const *d_in, void *const *d_out, const size_t *units,
                     void *producer_stream, long *ticket);
/* The root-device stream on which the NEXT pushed frame's kernels will run (NULL on processes that do not drive the
 * root).  A producer that enqueues the frame's inputs on this stream and passes it as producer_stream needs no event:
 * stream order already puts the frame's kernels behind it (one event record and one stream wait less per frame). */
void *xNodeStreamNextSlotStream(x266hip_nstream *s);
/* Issues the two draining steps and blocks until every pushed frame's results are in place. */
int  xNodeStreamFlush(x266hip_nstream *s);
/* Blocks the host until the results of step `ticket` are complete in their d_out buffers (root), or
 * the step's shard has left (peers).  No communication; EINVAL when fewer than two later steps exist. */
int  xNodeStreamWait(x266hip_nstream *s, long ticket);
/* One batch through the same machinery (SURVEY 8e "end-to-end scatter -> compute -> gather"): the batch
 * is cut into chunks of chunk_units (0 = default: one launch with one rank, else 8 MiB of input per
 * rank and chunk but at least four chunks), pushed as frames, flushed.  Synchronous.  d_in / d_out on the root as above. */
int  xNodeBatchScatterGather(x266hip_node *node, int op, const void *d_in, void *d_out, size_t n_units,
                             size_t chunk_units);
/* Full-search motion estimation of one frame over the node (xSatd8x8SearchDev semantics and argument
 * meaning; d_cur / d_ref / d_best on the root's device, NULL elsewhere): the frame is cut into
 * n_stripes horizontal stripes (0: one per rank) dealt to the ranks in contiguous runs; the root sends
 * each stripe of `cur` and the stripe's rows +- range of the padded reference, every rank searches its
 * stripes, the (mv, cost) records return to d_best.  Results are identical to the single-device call
 * for any n_stripes.  Synchronous. */
int  xNodeSatd8x8Search(x266hip_node *node, const uint8_t *d_cur, intptr_t cur_stride, const uint8_t *d_ref,
                        intptr_t ref_stride, int width, int height, int range, int n_stripes,
                        x266_me_result_t *d_best);

/* ------------------------------------------------------------------------ */
/* host-only utilities (no device needed)                                     */
/* ------------------------------------------------------------------------ */
/* BDPI packing of two input rows, Vector#(2,Vector#(32,Bit#(16))):
 * res[w] = (x[2w+1] << 16) + x[2w], row `first_row` then `first_row+1`
 * (src_tb/dct32.c:205-220). */
void     xDct32PackDiffRows(const int16_t *mat, int first_row, unsigned int res[32]);
/* BDPI packing of 4 vertically adjacent coefficients, column-major walk:
 * idx -> col = idx>>5, row = idx&31 (src_tb/dct32.c:223-246). */
uint64_t xDct32PackDctWord(const int16_t *dct, int idx);
/* The N x N matrix the transform-set kernels use for a 1-D transform: type 0 = DCT-II (rows 0, 32/N, ... of g_t32,
 * first N columns: the taps of src/mkDct32.bsv:132-141), 1 = DST-VII; N in {4, 8, 16} (and 32 for DCT-II).
 * m[k*N + n], row k = frequency.  Lets a host (and the CPU tests) check the product's own tables. */
int      xTransformMatrix(int type, int size, int16_t *m);
/* The order in which a host coder walks a size x size block of the compact level stream (xLevelsPackGpu): for size in {4, 8, 16, 32}
 * pos[s * 16 + i] = v * size + u of scan position i of CG s, size * size entries; X266HIP_EINVAL for any other size or a NULL pos. */
int      xLevelScan(int size, uint16_t *pos);
/* Regions the offset scan of xLevelsPackGpu takes per step (a test walks region counts around it). */
unsigned xLevelsScanChunk(void);
/* The rate model of xRdoQuantRegionsGpu / xLevelsBitsGpu, in 1/16 bit, from the very functions the kernels use: with them a host
 * coder or a rate control reproduces `bits`.  xLevelBits: R(abs_level, pos_class), abs_level 0..32768, pos_class 0..2.  xLastPosBits:
 * Rlast(u, v) of a block of 1 << log2_size, log2_size 2..5, u and v below the size.  xCgFlagBits: cgf[coded], coded 0 or 1.  Each
 * returns -1 for any other argument. */
int      xLevelBits(int abs_level, int pos_class);
int      xLastPosBits(int u, int v, int log2_size);
int      xCgFlagBits(int coded);
const char *xHipVersion(void);

/* ------------------------------------------------------------------------ */
/* BDPI drop-in surface (stateful, non-reentrant, single-threaded -- exactly  */
/* like upstream; device from env X266HIP_DEVICE, default 0)                  */
/* ------------------------------------------------------------------------ */
/* const int16_t g_t32[32][32]        -- src_tb/dct32.c:30 (exported global)  */
#ifndef X266HIP_DEFINING_TABLE   /* the defining TU generates it at compile time */
extern const int16_t g_t32[32][32];
#endif
/* draws a new 32x32 stimulus block with rand() and transforms it on the GPU  */
void               dct32_genNew(void);                    /* src_tb/dct32.c:178 */
/* two input rows per call, 16 calls per block                                */
void               dct32_getDiff(unsigned int res[]);     /* src_tb/dct32.c:205 */
/* four coefficients per call, column-major, 256 calls per block              */
unsigned long long dct32_getDct(void);                    /* src_tb/dct32.c:223 */
void               satd8x8_genNew(void);                  /* src_tb/satd.c:124  */
/* one row (8 x int16 = 4 words) per call                                     */
void               satd8x8_getDiff(unsigned int res[]);   /* src_tb/satd.c:143  */
unsigned int       satd8x8_getSatd(void);                 /* src_tb/satd.c:149  */
/* Per-call twin of the RISC-V benchmark's sad() (riscv/programs/benchmarks/sad/sad.c:28-39): same arguments and
 * result, on the GPU, through the same lazily created context; n in {4, 8, 16, 32, 64}, -1 otherwise. */
int                x266_sad(const unsigned char *input_data1, const unsigned char *input_data2, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* X266HIP_H */
