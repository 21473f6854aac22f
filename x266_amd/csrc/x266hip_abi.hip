// x266hip_abi.hip -- host side of libx266hip.so: context, batch entry points,
// device-memory helpers and kernel timing behind the C ABI of include/x266hip.h.
//
// Conventions follow src/x266.cpp (xCodecInit/xCodecFree :494-524: context
// struct first, caller-owned buffers, int 0 / negative returns, no exceptions
// across the boundary).  There is deliberately NO CPU fallback: every compute
// entry point needs a gfx950 device and fails loudly without one.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/x266hip.h"
#include "x266_aq.hpp"
#include "x266_args.hpp"
#include "x266_device.hpp"
#include "x266_entropy.hpp"
#include "x266_entropy_motion.hpp"
#include "x266_entropy_side.hpp"
#include "x266_levels.hpp"
#include "x266_motion.hpp"
#include "x266_quality.hpp"
#include "x266_rdoq.hpp"
#include "x266_lookahead.hpp"
#include "x266_tables.hpp"

using namespace x266;

struct x266hip_ctx {
    int device = 0;
    hipDeviceProp_t prop{};
    DctOps *d_fwd = nullptr;
    DctOps *d_inv_lds = nullptr;                    // inverse operand images for the LDS-staged kernel (column reads)
    DctOps *d_inv_acc = nullptr;                    // the same with pass A's K-slots in accumulator-row order (fused kernel: the inverse is fed from the forward's registers)
    static constexpr int kTypes = 4;                // DCT-II, DST-VII, and the two mixed horizontal / vertical pairs
    DctOps *d_tr[kTypes][3] = {};                   // [type][log2N - 2], N = 4, 8, 16
    DctOps *d_tr_inv[kTypes][3] = {};
    TileTab *d_tile_fwd = nullptr, *d_tile_inv = nullptr;      // the set's 1-D matrices in compact form, as is / transposed (xTransformTilesDev)
    // the two 1-D transform slots of the set, N = 4, 8, 16: slot 0 = DCT-II sub-matrices of g_t32, slot 1 = closed-form
    // DST-VII unless the caller installed its own (xTransformSetMatrix); row k = basis function, N x N, row-major
    int8_t slot_mat[2][3][256] = {};
    int slot1_preset = X266_PRESET_CLOSED_FORM;     // -1 once the caller installed a matrix of its own in slot 1
    bool tr_tables_valid = true;                    // false after a matrix update whose device tables could be neither installed nor rolled back
    // Launch options (xHipSetOption): A/B knobs, results never depend on them.  Defaults = the measured optimum.
    int dct_variant = 0;                            // 0 = matrix-core kernel, 2 = VALU butterfly (the comparison variant north_star asks for)
    int satd_variant = 0;                           // 0 = by batch size (staged kernel below 3 Mi blocks, LDS-DMA kernel from there), 1 = staged, 2 = VALU butterfly, 3 = LDS-DMA
    int dct_blocks_per_wave = 1, dct_inv_blocks_per_wave = 2, dct_fwdinv_blocks_per_wave = 0;   // consecutive blocks one wave loops over (profiles/r01_launch_sweep.txt)
    int satd_groups_per_wave = 0, satd_wg_threads = 0, satd_lds_per_wave = 0;                   // 0 = the chosen SATD kernel's own default (satd_kernels.hip, launch_satd8x8)
    int adaptive_per_wave = 1;                      // shrink the per-wave run on small batches
    int dct_wg_threads = 0;                         // workgroup size of the DCT32 / transform-set kernels; 0 = the measured best: one-wave workgroups (profiles/r01_wg_occupancy.txt), four-wave ones for the fused forward + inverse kernel (profiles/r05_fused_variants.txt)
    int tile_tiles_per_wave = 0;                    // mixed-class tile kernel: consecutive tiles per wave (0 = 2: the wave's table copy serves two tiles)
    int autotune = 0;                               // 1: the first large batch of a kernel family times its box-dependent launch shapes on the caller's buffers and keeps the fastest (tune_family below); 2 + k: every family launches candidate k, untimed (the tests' hook)
    int me_tile_rows = 0;                           // block rows per ME tile: 0 = by frame size (SATD search: 8, 4 or 2; SAD search: 2), else 2, 4, 8 (8: SATD search only; 1 is served by 2)
    // fixed launch shapes (options in rounds 1-3; their sweeps are frozen in profiles/r01_*.txt, r03_tiles_one_launch.txt)
    static constexpr int kDctLdsPerWave = 8192;     // 2 KiB used: at most 20 resident waves per CU
    static constexpr int kDctInvLdsPerWave = 10240; // the DCT32 inverse: 16
    static constexpr int kFwdInvLdsPerWave = 12288; // fused forward + inverse: 6 KiB used (two DMA slots + the converter): 12 resident waves per CU
    static constexpr int kTileLdsPerWave = 8192;    // table + two tile slots = 6 KiB used
    static constexpr int kIntraRounds = 4;          // intra prediction: rounds of seven predictions per wave
    // Internal device scratch, ONE BUFFER PER STREAM AND KIND, so that calls enqueued on different streams never share it:
    // kind 0 = motion search (128 B per 8x8 block of the current frame).  Each table is bounded (kMeScratchMax streams, least recently used evicted after waiting for its
    // last use); a buffer that was handed out during a stream capture may be referenced by a recorded graph and is kept
    // until the context is freed (outgrown ones are retired, not released).
    struct MeScratch {
        hipStream_t stream;
        uint32_t *p;
        size_t bytes;
        hipEvent_t last_use;
        unsigned long long stamp;
        bool pinned;
        bool capturing_now;
    };
    // "autotune": per kernel family the chosen candidate (-1 = not tuned yet) and what every candidate measured
    enum { kTuneFwdInv, kTuneRecon, kTuneSatd, kTuneSad8, kTuneSad16, kTuneSad32, kTuneSad64, kTuneFamilies };
    static constexpr int kTuneMaxCands = 8;
    struct Tuned { int choice = -1; int n = 0; float ms[kTuneMaxCands] = {}; };
    Tuned tuned[kTuneFamilies];
    // "autotune" = 2 + k: per family the candidate its forced launches took (-1 = none yet) and how many there were (xHipAutotuneReport)
    struct Forced { int cand = -1; unsigned long long launches = 0; };
    Forced forced[kTuneFamilies];
    hipEvent_t tune_ev[2] = {};
    static constexpr size_t kMeScratchMax = 8;
    static constexpr int kScratchKinds = 1;
    std::vector<MeScratch> scratch[kScratchKinds];
    std::vector<void *> me_retired;
    unsigned long long me_stamp = 0;
    // host-pointer staging (lazily allocated)
    static constexpr int kSlots = 3;                // chunk i+1 uploading and chunk i-1 downloading while chunk i is transformed
    void *d_stage_in[kSlots] = {};
    void *d_stage_out[kSlots] = {};
    size_t stage_in_bytes = 0, stage_out_bytes = 0;
    // one stream per ENGINE, not per slot: every upload on [0], every kernel on [1], every download on [2], ordered by the
    // slots' events.  With a stream per slot (rounds 1-3) uploads and downloads of different chunks did not overlap on this
    // runtime: 28-30 GB/s each way from pinned memory against 43 this way (profiles/r04_hostpipe.txt; the link gives 48.5 both ways)
    hipStream_t stage_stream[3] = {};
    // small host-pointer calls (the BDPI shims: one block per call): two page-locked, device-visible 64 KiB buffers the kernel reads and writes in place
    static constexpr size_t kSmallCallBytes = (size_t)64 << 10;
    void *h_small_in = nullptr, *h_small_out = nullptr;
    hipStream_t small_stream = nullptr;
    hipEvent_t stage_up[kSlots] = {}, stage_done[kSlots] = {}, stage_down[kSlots] = {};
    std::string err;
};

namespace {

int fail(x266hip_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) {
            ctx->err += ": ";
            ctx->err += hipGetErrorString(e);
        }
    }
    return code;
}

// a refused call: X266HIP_EINVAL and the text "<entry point>: <reason>" (the reasons: x266_args.hpp); nothing is launched
int refuse(x266hip_ctx *ctx, const char *entry, const char *why)
{
    ctx->err = entry;
    ctx->err += ": ";
    ctx->err += why;
    return X266HIP_EINVAL;
}

// the tail of every entry point: the launch's status as the return code
int launched(x266hip_ctx *ctx, const char *what, hipError_t e) { return e == hipSuccess ? X266HIP_OK : fail(ctx, X266HIP_EDEVICE, what, e); }

int tables_invalid(x266hip_ctx *ctx, const char *entry)
{
    return fail(ctx, X266HIP_EDEVICE, (std::string(entry) + ": the transform tables of this context are invalid (a failed xTransformSetMatrix)").c_str());
}

#define X_HIP(ctx, call)                                                     \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return fail((ctx), X266HIP_EDEVICE, #call, e_); \
    } while (0)

// Every entry point runs on the context's device and puts the caller's current device back on return
// (a host that also drives other GPUs, or torch with another current device, is not retargeted).
struct DeviceScope {
    int prev = -1;
    hipError_t status;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        status = prev == dev ? hipSuccess : hipSetDevice(dev);
        if (prev == dev) prev = -1;                                    // nothing to restore
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define X_DEV(ctx)                                                            \
    DeviceScope dev_scope_((ctx)->device);                                    \
    if (dev_scope_.status != hipSuccess) return fail((ctx), X266HIP_EDEVICE, "hipSetDevice", dev_scope_.status)

LaunchCfg cfg_for(const x266hip_ctx *ctx, int op)
{
    LaunchCfg c;
    c.cu_count = ctx->prop.multiProcessorCount;
    c.adaptive = ctx->adaptive_per_wave;
    if (op == 2) {
        c.units_per_wave = ctx->satd_groups_per_wave;
        c.wg_threads = ctx->satd_wg_threads;
        c.lds_bytes_per_wave = ctx->satd_lds_per_wave;
        c.shape = ctx->satd_variant == 1 || ctx->satd_variant == 3 ? ctx->satd_variant : 0;
    } else {
        c.units_per_wave = op == 1 ? ctx->dct_inv_blocks_per_wave : ctx->dct_blocks_per_wave;
        c.wg_threads = ctx->dct_wg_threads ? ctx->dct_wg_threads : 64;
        c.lds_bytes_per_wave = x266hip_ctx::kDctLdsPerWave;

        c.shape = 0;
    }
    return c;
}

int launch_op(x266hip_ctx *ctx, int op, const void *d_in, void *d_out, size_t n, hipStream_t s)
{
    hipError_t e;
    switch (op) {
    case 0:
        if (ctx->dct_variant == 2) e = launch_dct32_butterfly((const int16_t *)d_in, (int16_t *)d_out, n, s);   // VALU comparison variant
        else e = launch_dct32(false, (const int16_t *)d_in, (int16_t *)d_out, n, ctx->d_fwd, cfg_for(ctx, 0), s);
        break;
    case 1: {
        // the inverse does more arithmetic per tile than the forward: 10 KiB charged per wave = 16 resident waves per CU instead of 20 (paired sweep in one process: -1.8 %;
        // the forward, the small transforms and their inverses keep 8 KiB, tools/probes/gpu_dct_family_shapes.py)
        LaunchCfg cfg = cfg_for(ctx, 1);
        cfg.lds_bytes_per_wave = x266hip_ctx::kDctInvLdsPerWave;
        e = launch_dct32(true, (const int16_t *)d_in, (int16_t *)d_out, n, ctx->d_inv_lds, cfg, s);
        break;
    }
    case 2:
        if (ctx->satd_variant == 2) e = launch_satd8x8_butterfly((const int16_t *)d_in, (uint32_t *)d_out, n, cfg_for(ctx, 2), s);   // VALU comparison variant
        else e = launch_satd8x8((const int16_t *)d_in, (uint32_t *)d_out, n, cfg_for(ctx, 2), s);
        break;
    case 3: case 4: case 5: case 6: e = launch_mem_ceiling(op - 3, d_in, d_out, n * 2048, s); break;      // xHipTimeKernel only
    default: return fail(ctx, X266HIP_EINVAL, "unknown op");
    }
    if (e != hipSuccess) return fail(ctx, X266HIP_EDEVICE, "kernel launch", e);
    return X266HIP_OK;
}

// ---- opt-in launch-shape autotuning ("autotune" = 1; off by default; results never depend on it) ---------------------------
// Boxes of the pool differ in which launch shape a few kernels run fastest in (profiles/r05_fused_variants.txt: the fused forward +
// inverse kernel's best shape is a different one on four of six boxes, up to 5 % apart).  With the option on, the FIRST call of a
// family whose batch is large enough to time (the caller says so by `big`) runs every candidate on the caller's own buffers and
// stream -- one warm-up and three timed launches each, HIP events on that stream, so this one call is synchronous -- and the
// context keeps the fastest; the default shape (candidate 0) stays unless another one beats it by more than 2 %.  Every candidate
// writes the same bytes, so the extra launches only rewrite the outputs.  The tuning call's last launch overwrites what the others wrote, so
// comparing its outputs checks the kept shape alone (tests/test_gpu_autotune.py: option off / on per family); each candidate by itself is
// checked through "autotune" = 2 + k, which launches candidate k of every family at any batch size, untimed: tests/test_gpu_launch_shapes.py
// holds every entry of the four tables against the CPU oracle at the run lengths where the pipelines switch cases, inside guard bands, and
// tests/test_gpu_waits.py every fused entry against the wait-for-everything build.
// Not while the stream is being captured, and not for calls whose buffers overlap (the caller checks): those use the default.
template <class Launch>
int tune_family(x266hip_ctx *ctx, int family, int n_cands, bool big, hipStream_t stream, Launch &&launch)
{
    x266hip_ctx::Tuned &t = ctx->tuned[family];
    if (!ctx->autotune) return 0;
    if (t.choice >= 0) return t.choice;
    if (!big) return 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cap);
    (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone) return 0;
    for (hipEvent_t &e : ctx->tune_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; (void)hipGetLastError(); return 0; }
    if (n_cands > x266hip_ctx::kTuneMaxCands) n_cands = x266hip_ctx::kTuneMaxCands;
    t.n = n_cands;
    int best = 0;
    for (int c = 0; c < n_cands; ++c) {
        t.ms[c] = -1.f;
        if (launch(c) != hipSuccess) { (void)hipGetLastError(); continue; }
        bool ok = hipEventRecord(ctx->tune_ev[0], stream) == hipSuccess;
        for (int r = 0; ok && r < 3; ++r) ok = launch(c) == hipSuccess;
        float ms = 0.f;
        ok = ok && hipEventRecord(ctx->tune_ev[1], stream) == hipSuccess && hipEventSynchronize(ctx->tune_ev[1]) == hipSuccess &&
             hipEventElapsedTime(&ms, ctx->tune_ev[0], ctx->tune_ev[1]) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); continue; }
        t.ms[c] = ms / 3.f;
        if (c && t.ms[c] > 0.f && (t.ms[best] <= 0.f || t.ms[c] < t.ms[best])) best = c;
    }
    if (best && t.ms[0] > 0.f && t.ms[best] > 0.98f * t.ms[0]) best = 0;   // within 2 % of the default (run-to-run noise is ~1 %): keep the default
    t.choice = best;
    return best;
}

struct ShapeCand {
    int units_per_wave, wg_threads, lds_bytes_per_wave, shape;
    LaunchCfg over(LaunchCfg c) const { c.units_per_wave = units_per_wave; c.wg_threads = wg_threads; c.lds_bytes_per_wave = lds_bytes_per_wave; c.shape = shape; return c; }
};
// fused forward + inverse with both outputs: the default first, then the deep long-lived shapes of profiles/r05_fused_variants.txt
const ShapeCand kFwdInvCands[] = {{2, 256, 12288, 2}, {16, 256, 16384, 3}, {24, 256, 16384, 3}, {16, 128, 20480, 3}, {12, 256, 16384, 3}, {4, 128, 12288, 2},
                                  {16, 256, 16384, 4}, {4, 64, 16384, 3}};
const ShapeCand kReconCands[] = {{8, 256, 12288, 2}, {4, 256, 12288, 2}, {16, 256, 16384, 3}, {8, 128, 12288, 2}, {6, 256, 12288, 2}};
// SATD batch, LDS-DMA kernel (groups per wave, workgroup, LDS per wave)
const ShapeCand kSatdCands[] = {{4, 256, 16384, 3}, {2, 256, 16384, 3}, {8, 256, 16384, 3}, {4, 128, 12288, 3}, {6, 256, 12288, 3}, {3, 256, 12288, 3}};
// SAD batch: (-, waves per workgroup x 64, LDS per WORKGROUP)
const ShapeCand kSadCands[] = {{0, 256, 32768, 0}, {0, 128, 16384, 0}, {0, 64, 8192, 0}, {0, 256, 24576, 0}, {0, 256, 40960, 0}};

// "autotune" = 2 + k (the tests' hook): the candidate every family is to launch, -1 when the option does not force one
int forced_cand(const x266hip_ctx *ctx) { return ctx->autotune >= 2 ? ctx->autotune - 2 : -1; }
void count_forced(x266hip_ctx *ctx, int family, int cand)
{
    ctx->forced[family].cand = cand;
    ++ctx->forced[family].launches;
}

// One launch of a family under "autotune": the forced candidate (refused when it is past the family's table), else the tuned one.
template <class Launch>
int run_family(x266hip_ctx *ctx, const char *entry, int family, int n_cands, bool big, hipStream_t stream, Launch &&run, hipError_t *e)
{
    const int forced = forced_cand(ctx);
    if (forced >= n_cands) return refuse(ctx, entry, "option \"autotune\" forces a launch shape this family does not have");
    *e = run(forced >= 0 ? forced : tune_family(ctx, family, n_cands, big, stream, run));
    if (forced >= 0 && *e == hipSuccess) count_forced(ctx, family, forced);
    return X266HIP_OK;
}

// the autotune paths only: calls whose buffers overlap take the default shape (the entry points' own rules: x266_args.hpp)
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

// Scratch of kind `kind` for `stream`, at least `need` bytes.  Allocation happens here, i.e. on the first call of a stream or
// size -- or ahead of time through xHipMeScratchReserve, which is what a host does before a stream
// capture or a real-time loop (hipMalloc is illegal under capture and synchronises).
int scratch_for(x266hip_ctx *ctx, int kind, hipStream_t stream, size_t need, x266hip_ctx::MeScratch **out)
{
    std::vector<x266hip_ctx::MeScratch> &table = ctx->scratch[kind];
    x266hip_ctx::MeScratch *slot = nullptr;
    for (x266hip_ctx::MeScratch &m : table)
        if (m.stream == stream) slot = &m;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cap);
    (void)hipGetLastError();
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (!slot) {
        if (table.size() >= x266hip_ctx::kMeScratchMax && !capturing) {          // evict the least recently used stream's buffer
            size_t victim = table.size();
            for (size_t i = 0; i < table.size(); ++i)
                if (!table[i].pinned && (victim == table.size() || table[i].stamp < table[victim].stamp)) victim = i;
            if (victim < table.size()) {
                x266hip_ctx::MeScratch &v = table[victim];
                if (v.last_use) { (void)hipEventSynchronize(v.last_use); (void)hipEventDestroy(v.last_use); }
                if (v.p) (void)hipFree(v.p);
                table.erase(table.begin() + (long)victim);
            }
        }
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        table.push_back({stream, nullptr, 0, ev, 0, false, false});
        slot = &table.back();
    }
    if (need > slot->bytes) {
        if (capturing) return fail(ctx, X266HIP_EINVAL, "internal scratch cannot be allocated under stream capture: reserve it (or run the call once) beforehand");
        void *fresh = nullptr;
        if (hipMalloc(&fresh, need) != hipSuccess) return fail(ctx, X266HIP_ENOMEM, "internal scratch");
        if (slot->p) {
            if (slot->pinned) ctx->me_retired.push_back(slot->p);        // a recorded graph may still use it
            else { if (slot->last_use) (void)hipEventSynchronize(slot->last_use); (void)hipFree(slot->p); }
        }
        slot->p = (uint32_t *)fresh;
        slot->bytes = need;
        slot->pinned = false;
    }
    if (capturing) slot->pinned = true;
    slot->capturing_now = capturing;
    slot->stamp = ++ctx->me_stamp;
    *out = slot;
    return X266HIP_OK;
}

// motion search: tile-major coefficient table of whole search tiles, partial edge tiles padded (tile heights 1, 2, 4, 8 all fit)
int me_scratch_for(x266hip_ctx *ctx, hipStream_t stream, int width, int height, x266hip_ctx::MeScratch **out)
{
    return scratch_for(ctx, 0, stream, (size_t)((width / 8 + 7) / 8) * 8 * (size_t)((height / 8 + 7) / 8) * 8 * 128, out);
}

// built-in matrix of a 1-D transform slot: 0 = DCT-II (rows 0, 32/N, ... of g_t32, first N columns), 1 = closed-form DST-VII
void default_slot_matrix(int slot, int n, int8_t *m)
{
    const Matrix32 d = make_transform_matrix(slot == 0 ? kTrDct2 : kTrDst7, n);
    for (int k = 0; k < n; ++k)
        for (int c = 0; c < n; ++c) m[k * n + c] = d.v[k][c];
}

Matrix32 block_diagonal(const int8_t *m, int n)
{
    Matrix32 r{};
    for (int k = 0; k < 32; ++k)
        for (int c = 0; c < 32; ++c) r.v[k][c] = k / n == c / n ? m[(k % n) * n + (c % n)] : (int8_t)0;
    return r;
}

typedef int8_t SlotMatrices[2][3][256];

// operand images of class (type, N = 4 << l) from a set of slot matrices: the two per-class tables (allocated on first use)
bool upload_class(x266hip_ctx *ctx, const SlotMatrices &mat, int type, int l, DctOps *h)
{
    const int n = 4 << l;
    const Matrix32 mh = block_diagonal(mat[transform_htype(type) == kTrDst7][l], n);
    const Matrix32 mv = block_diagonal(mat[transform_vtype(type) == kTrDst7][l], n);
    build_fwd_ops_general(*h, mh, mv, transform_shift1(n), transform_shift2(n));
    if (!ctx->d_tr[type][l] && hipMalloc((void **)&ctx->d_tr[type][l], sizeof(DctOps)) != hipSuccess) return false;
    if (hipMemcpy(ctx->d_tr[type][l], h, sizeof(DctOps), hipMemcpyHostToDevice) != hipSuccess) return false;
    build_inv_ops_general(*h, mv, mh);
    if (!ctx->d_tr_inv[type][l] && hipMalloc((void **)&ctx->d_tr_inv[type][l], sizeof(DctOps)) != hipSuccess) return false;
    return hipMemcpy(ctx->d_tr_inv[type][l], h, sizeof(DctOps), hipMemcpyHostToDevice) == hipSuccess;
}

// the mixed-class tile kernel's compact tables from a set of slot matrices
bool upload_tile_tabs(x266hip_ctx *ctx, const SlotMatrices &mat)
{
    TileTab t;
    build_tile_tab(t, mat, false);
    if (hipMemcpy(ctx->d_tile_fwd, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) return false;
    build_tile_tab(t, mat, true);
    return hipMemcpy(ctx->d_tile_inv, &t, sizeof t, hipMemcpyHostToDevice) == hipSuccess;
}

// every device table that depends on (slot, N = 4 << l) of `mat`
bool upload_slot_tables(x266hip_ctx *ctx, const SlotMatrices &mat, int slot, int l, DctOps *h)
{
    for (int type = 0; type < x266hip_ctx::kTypes; ++type)
        if ((transform_htype(type) == kTrDst7) == (slot == 1) || (transform_vtype(type) == kTrDst7) == (slot == 1))
            if (!upload_class(ctx, mat, type, l, h)) return false;
    return upload_tile_tabs(ctx, mat);
}

}  // namespace

extern "C" {

const char *xHipVersion(void) { return "x266hip 0.1 (gfx950)"; }

int xHipDeviceCount(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

int xHipCodecInit(x266hip_ctx **out, int device_id)
{
    if (!out) return X266HIP_EINVAL;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        std::fprintf(stderr, "x266hip: no HIP device available (this library has no CPU path)\n");
        return X266HIP_EDEVICE;
    }
    if (device_id < 0 || device_id >= n_dev) return X266HIP_EINVAL;
    x266hip_ctx *ctx = new (std::nothrow) x266hip_ctx;
    if (!ctx) return X266HIP_ENOMEM;
    ctx->device = device_id;
    DeviceScope dev_scope_(device_id);
    if (dev_scope_.status != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess) {
        delete ctx;
        return X266HIP_EDEVICE;
    }
    if (std::strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "x266hip: device %d is %s; the kernels are built for gfx950 only\n", device_id,
                     ctx->prop.gcnArchName);
        delete ctx;
        return X266HIP_EDEVICE;
    }
    DctOps *h = new (std::nothrow) DctOps;
    bool ok = h != nullptr;
    if (ok) ok = hipMalloc((void **)&ctx->d_fwd, sizeof(DctOps)) == hipSuccess;
    if (ok) {
        build_fwd_ops(*h);
        ok = hipMemcpy(ctx->d_fwd, h, sizeof(DctOps), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        build_inv_ops(*h, true);
        ok = hipMalloc((void **)&ctx->d_inv_lds, sizeof(DctOps)) == hipSuccess &&
             hipMemcpy(ctx->d_inv_lds, h, sizeof(DctOps), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        build_inv_ops(*h, false);
        ok = hipMalloc((void **)&ctx->d_inv_acc, sizeof(DctOps)) == hipSuccess &&
             hipMemcpy(ctx->d_inv_acc, h, sizeof(DctOps), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        for (int slot = 0; slot < 2; ++slot)
            for (int l = 0; l < 3; ++l) default_slot_matrix(slot, 4 << l, ctx->slot_mat[slot][l]);
        ok = hipMalloc((void **)&ctx->d_tile_fwd, sizeof(TileTab)) == hipSuccess &&
             hipMalloc((void **)&ctx->d_tile_inv, sizeof(TileTab)) == hipSuccess;
    }
    for (int type = 0; type < x266hip_ctx::kTypes && ok; ++type)
        for (int l = 0; l < 3 && ok; ++l) ok = upload_class(ctx, ctx->slot_mat, type, l, h);
    if (ok) ok = upload_tile_tabs(ctx, ctx->slot_mat);
    delete h;

    if (!ok) {
        xHipCodecFree(ctx);
        return X266HIP_ENOMEM;
    }
    *out = ctx;
    return X266HIP_OK;
}

void xHipCodecFree(x266hip_ctx *ctx)
{
    if (!ctx) return;
    DeviceScope dev_scope_(ctx->device);
    for (int i = 0; i < x266hip_ctx::kSlots; ++i) {
        if (ctx->d_stage_in[i]) (void)hipFree(ctx->d_stage_in[i]);
        if (ctx->d_stage_out[i]) (void)hipFree(ctx->d_stage_out[i]);
        if (ctx->stage_up[i]) (void)hipEventDestroy(ctx->stage_up[i]);
        if (ctx->stage_done[i]) (void)hipEventDestroy(ctx->stage_done[i]);
        if (ctx->stage_down[i]) (void)hipEventDestroy(ctx->stage_down[i]);
    }
    for (hipStream_t st : ctx->stage_stream)
        if (st) (void)hipStreamDestroy(st);
    if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
    if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
    if (ctx->small_stream) (void)hipStreamDestroy(ctx->small_stream);
    for (int type = 0; type < x266hip_ctx::kTypes; ++type)
        for (int l = 0; l < 3; ++l) {
            if (ctx->d_tr[type][l]) (void)hipFree(ctx->d_tr[type][l]);
            if (ctx->d_tr_inv[type][l]) (void)hipFree(ctx->d_tr_inv[type][l]);
        }
    for (auto &table : ctx->scratch)
        for (const x266hip_ctx::MeScratch &m : table) { if (m.p) (void)hipFree(m.p); if (m.last_use) (void)hipEventDestroy(m.last_use); }
    for (void *q : ctx->me_retired) (void)hipFree(q);
    for (hipEvent_t e : ctx->tune_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->d_tile_fwd) (void)hipFree(ctx->d_tile_fwd);
    if (ctx->d_tile_inv) (void)hipFree(ctx->d_tile_inv);
    if (ctx->d_fwd) (void)hipFree(ctx->d_fwd);
    if (ctx->d_inv_lds) (void)hipFree(ctx->d_inv_lds);
    if (ctx->d_inv_acc) (void)hipFree(ctx->d_inv_acc);
    delete ctx;
}

const char *xHipLastError(const x266hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// The chip's name for humans.  hipDeviceProp_t::name is EMPTY on this pool's ROCm 7.2 boxes (BENCH_r05's "device" read
// "(gfx950:sramecc+:xnack-)"), so ask in turn: the property, hipDeviceGetName, the amdgpu driver's product_name in sysfs,
// and last a table keyed on what the property block does carry (arch, CU count, peak clock) -- marked as such.
static std::string device_marketing_name(const x266hip_ctx *ctx)
{
    auto trimmed = [](const char *s) {
        std::string t(s ? s : "");
        while (!t.empty() && (t.back() == ' ' || t.back() == '\n' || t.back() == '\r' || t.back() == '\t')) t.pop_back();
        size_t b = 0;
        while (b < t.size() && t[b] == ' ') ++b;
        return t.substr(b);
    };
    std::string n = trimmed(ctx->prop.name);
    if (!n.empty()) return n;
    char buf[256] = {0};
    if (hipDeviceGetName(buf, sizeof buf - 1, ctx->device) == hipSuccess && !(n = trimmed(buf)).empty()) return n;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus - 1, ctx->device) == hipSuccess) {
        for (char *c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
        const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/product_name";
        if (FILE *f = std::fopen(path.c_str(), "r")) {
            const bool got = std::fgets(buf, sizeof buf, f) != nullptr;
            std::fclose(f);
            if (got && !(n = trimmed(buf)).empty()) return n;
        }
    }
    const std::string arch(ctx->prop.gcnArchName);
    if (arch.rfind("gfx950", 0) == 0 && ctx->prop.multiProcessorCount == 256)       // the two 256-CU gfx950 parts differ in peak clock
        return ctx->prop.clockRate >= 2300000 ? "AMD Instinct MI355X [by arch/CU/clock table]" : "AMD Instinct MI350X [by arch/CU/clock table]";
    return "unnamed AMD GPU";
}

int xHipDeviceInfo(const x266hip_ctx *ctx, char *name, size_t name_cap, int *cu_count, int *clock_mhz,
                   size_t *hbm_bytes)
{
    if (!ctx) return X266HIP_EINVAL;
    if (name && name_cap) {
        const std::string chip = device_marketing_name(ctx);
        std::snprintf(name, name_cap, "%s (%s)", chip.c_str(), ctx->prop.gcnArchName);
    }
    if (cu_count) *cu_count = ctx->prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = ctx->prop.clockRate / 1000;
    if (hbm_bytes) *hbm_bytes = ctx->prop.totalGlobalMem;
    return X266HIP_OK;
}

// One table for every launch option: key, the context member it sets, accepted range, and a
// required divisor (workgroup sizes are whole waves).
struct OptionDesc {
    const char *key;
    int x266hip_ctx::*member;
    int lo, hi, multiple_of;
};

static const OptionDesc kOptions[] = {
    {"adaptive_per_wave", &x266hip_ctx::adaptive_per_wave, 0, 1, 1},
    {"dct32_variant", &x266hip_ctx::dct_variant, 0, 2, 2},          // 0 or 2
    {"satd_variant", &x266hip_ctx::satd_variant, 0, 3, 1},
    {"dct32_blocks_per_wave", &x266hip_ctx::dct_blocks_per_wave, 1, 4096, 1},
    {"dct32_inv_blocks_per_wave", &x266hip_ctx::dct_inv_blocks_per_wave, 1, 4096, 1},
    {"dct32_fwdinv_blocks_per_wave", &x266hip_ctx::dct_fwdinv_blocks_per_wave, 0, 4096, 1},   // 0 = automatic: 2, and 8 when only the reconstruction is wanted
    {"dct32_wg_threads", &x266hip_ctx::dct_wg_threads, 0, 256, 64},
    {"satd_groups_per_wave", &x266hip_ctx::satd_groups_per_wave, 0, 4096, 1},
    {"satd_wg_threads", &x266hip_ctx::satd_wg_threads, 0, 256, 64},
    {"satd_lds_bytes_per_wave", &x266hip_ctx::satd_lds_per_wave, 0, 16384, 16},      // whole 16-byte rows; 16 KiB x the four waves of the largest workgroup = the 64 KiB a launch may ask for
    {"tile_tiles_per_wave", &x266hip_ctx::tile_tiles_per_wave, 0, 64, 1},
    {"me_tile_rows", &x266hip_ctx::me_tile_rows, 0, 8, 1},
    {"autotune", &x266hip_ctx::autotune, 0, 2 + x266hip_ctx::kTuneMaxCands, 1},           // 2 + k forces candidate k; a k past a family's table (k = 8: past every table) is refused by that family's calls
};

static const OptionDesc *find_option(const char *key)
{
    if (!key) return nullptr;
    for (const OptionDesc &o : kOptions)
        if (!std::strcmp(key, o.key)) return &o;
    return nullptr;
}

int xHipSetOption(x266hip_ctx *ctx, const char *key, int value)
{
    if (!ctx) return X266HIP_EINVAL;
    const OptionDesc *o = find_option(key);
    if (!o) return fail(ctx, X266HIP_EINVAL, "unknown option");
    if (value < o->lo || value > o->hi || value % o->multiple_of) return fail(ctx, X266HIP_EINVAL, "option value out of range");
    ctx->*(o->member) = value;
    if (o->member == &x266hip_ctx::autotune)                                   // any value: what was tuned or forced so far is forgotten
        for (int f = 0; f < x266hip_ctx::kTuneFamilies; ++f) { ctx->tuned[f] = x266hip_ctx::Tuned(); ctx->forced[f] = x266hip_ctx::Forced(); }
    return X266HIP_OK;
}

int xHipGetOption(const x266hip_ctx *ctx, const char *key, int *value)
{
    const OptionDesc *o = find_option(key);
    if (!ctx || !o || !value) return X266HIP_EINVAL;
    *value = ctx->*(o->member);
    return X266HIP_OK;
}

int xHipAutotuneReport(const x266hip_ctx *ctx, char *buf, size_t cap)
{
    if (!ctx || !buf || !cap) return X266HIP_EINVAL;
    static const char *const names[x266hip_ctx::kTuneFamilies] = {"dct32_fwd_inv", "dct32_recon_only", "satd8x8", "sad8", "sad16", "sad32", "sad64"};
    std::string out;
    char line[160];
    for (int f = 0; f < x266hip_ctx::kTuneFamilies; ++f) {
        const x266hip_ctx::Tuned &t = ctx->tuned[f];
        if (ctx->forced[f].cand >= 0) {
            std::snprintf(line, sizeof line, "%s forced %d launches %llu\n", names[f], ctx->forced[f].cand, ctx->forced[f].launches);
            out += line;
        }
        if (t.choice < 0) continue;
        std::snprintf(line, sizeof line, "%s choice %d ms", names[f], t.choice);
        out += line;
        for (int c = 0; c < t.n; ++c) { std::snprintf(line, sizeof line, " %.4f", t.ms[c]); out += line; }
        out += "\n";
    }
    if (out.size() >= cap) { buf[0] = '\0'; return X266HIP_EINVAL; }           // never a cut line
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return X266HIP_OK;
}

// ---- device-pointer API --------------------------------------------------------
// Every entry point: NULL context, the call's rule function (x266_args.hpp: a refused call launches nothing), context state,
// the device, the launch, `launched`.
int xDct32FwdBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::batch(d_in, d_out, 16, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launch_op(ctx, 0, d_in, d_out, n, (hipStream_t)stream);
}

int xDct32InvBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::batch(d_in, d_out, 16, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launch_op(ctx, 1, d_in, d_out, n, (hipStream_t)stream);
}

int xDct32SatdFrameDev(x266hip_ctx *ctx, const int16_t *d_dct_in, int16_t *d_dct_out, size_t n_dct_blocks,
                       const int16_t *d_diff, uint32_t *d_satd_out, size_t n_satd_blocks, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::dct32_satd_frame(d_dct_in, d_dct_out, n_dct_blocks, d_diff, d_satd_out, n_satd_blocks)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "frame lanes launch",
                    launch_frame_lanes(d_dct_in, d_dct_out, n_dct_blocks, ctx->d_fwd, d_diff, d_satd_out, n_satd_blocks, cfg_for(ctx, 2), (hipStream_t)stream));
}

int xDct32PassDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_out, size_t n, int shift, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::dct32_pass(d_in, d_out, n, shift)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "1-D pass launch", launch_dct32_pass(d_in, d_out, n, shift, ctx->d_fwd, (hipStream_t)stream));
}

int xDct32FwdInvBatchDev(x266hip_ctx *ctx, const int16_t *d_in, int16_t *d_coef, int16_t *d_recon, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::dct32_fwd_inv_batch(d_in, d_coef, d_recon, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    LaunchCfg cfg = cfg_for(ctx, 1);
    // 2 blocks per wave with both outputs (the shape that held 0.73-0.76 of 8 TB/s on every box); without the coefficient output the wave's traffic is a
    // third less and its arithmetic the same: 8 blocks per wave (paired over four boxes x three allocations, profiles/r05_fused_variants.txt: 2 -> 4 -8 %, 4 -> 8 another -1 to -4 %)
    cfg.units_per_wave = ctx->dct_fwdinv_blocks_per_wave ? ctx->dct_fwdinv_blocks_per_wave : (d_coef ? 2 : 8);
    if (!ctx->dct_wg_threads) cfg.wg_threads = 256;
    cfg.lds_bytes_per_wave = x266hip_ctx::kFwdInvLdsPerWave;
    cfg.shape = 2;
    hipError_t e;
    const bool knobs_untouched = !ctx->dct_fwdinv_blocks_per_wave && !ctx->dct_wg_threads;
    const bool disjoint = !ranges_overlap(d_in, n * 2048, d_recon, n * 2048) && !ranges_overlap(d_in, n * 2048, d_coef, n * 2048);
    if (ctx->autotune && n && knobs_untouched && disjoint) {
        const ShapeCand *cands = d_coef ? kFwdInvCands : kReconCands;
        const int n_cands = d_coef ? (int)(sizeof kFwdInvCands / sizeof kFwdInvCands[0]) : (int)(sizeof kReconCands / sizeof kReconCands[0]);
        auto run = [&](int c) { return launch_dct32_fwdinv(d_in, d_coef, d_recon, n, ctx->d_fwd, ctx->d_inv_acc, cands[c].over(cfg), (hipStream_t)stream); };
        if (const int rc = run_family(ctx, __func__, d_coef ? x266hip_ctx::kTuneFwdInv : x266hip_ctx::kTuneRecon, n_cands, n >= ((size_t)1 << 18), (hipStream_t)stream, run, &e)) return rc;
    } else {
        e = launch_dct32_fwdinv(d_in, d_coef, d_recon, n, ctx->d_fwd, ctx->d_inv_acc, cfg, (hipStream_t)stream);
    }
    return launched(ctx, "fwd+inv launch", e);
}

int xSatd8x8BatchDev(x266hip_ctx *ctx, const int16_t *d_diff, uint32_t *d_out, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::batch(d_diff, d_out, 4, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    const bool knobs_untouched = !ctx->satd_variant && !ctx->satd_groups_per_wave && !ctx->satd_wg_threads && !ctx->satd_lds_per_wave;
    // forcing: at any size (the LDS-DMA kernel runs from one block on, as under "satd_variant" 3)
    if (ctx->autotune && knobs_untouched && (forced_cand(ctx) >= 0 ? n > 0 : n >= kSatdDmaMinBlocks) && !ranges_overlap(d_diff, n * 128, d_out, n * 4)) {
        auto run = [&](int c) { return launch_satd8x8(d_diff, d_out, n, kSatdCands[c].over(cfg_for(ctx, 2)), (hipStream_t)stream); };
        hipError_t e;
        if (const int rc = run_family(ctx, __func__, x266hip_ctx::kTuneSatd, (int)(sizeof kSatdCands / sizeof kSatdCands[0]), n >= ((size_t)1 << 23), (hipStream_t)stream, run, &e)) return rc;
        return launched(ctx, "kernel launch", e);
    }
    return launch_op(ctx, 2, d_diff, d_out, n, (hipStream_t)stream);
}

int xHipMemCeilingDev(x266hip_ctx *ctx, int kind, const void *d_src, void *d_dst, size_t bytes, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::mem_ceiling(kind, d_src, d_dst, bytes)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "memory ceiling launch", launch_mem_ceiling(kind, d_src, d_dst, bytes, (hipStream_t)stream));
}

int xIntra32PredictDev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_modes,
                       const uint32_t *d_ref_index, uint8_t *d_pred, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::intra32_predict(d_refs, d_modes, d_ref_index, d_pred, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "intra launch", launch_intra32_predict(d_refs, d_modes, d_ref_index, d_pred, n, x266hip_ctx::kIntraRounds, (hipStream_t)stream));
}

int xIntra32ResidualDct32Dev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_modes, const uint32_t *d_ref_index,
                             const uint8_t *d_src, int16_t *d_coef, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::intra32_residual_dct32(d_refs, d_modes, d_ref_index, d_src, d_coef, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "intra residual + transform launch", launch_intra32_residual_dct32(d_refs, d_modes, d_ref_index, d_src, d_coef, n, ctx->d_fwd, (hipStream_t)stream));
}

int xIntra32CostsDev(x266hip_ctx *ctx, const x266_intra_ref_t *d_refs, const uint8_t *d_src,
                     uint32_t *d_costs, uint8_t *d_best_mode, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::intra32_costs(d_refs, d_src, d_costs, d_best_mode, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "intra decision launch", launch_intra32_costs(d_refs, d_src, d_costs, d_best_mode, n, (hipStream_t)stream));
}

int xFillResidualDev(x266hip_ctx *ctx, int16_t *d_dst, size_t n_samples, uint64_t seed, uint64_t first_index,
                     void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::fill_residual(d_dst, n_samples)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fill launch", launch_fill_residual(d_dst, n_samples, seed, first_index, cfg_for(ctx, 0), (hipStream_t)stream));
}

static_assert(args::kTransformTypes == x266hip_ctx::kTypes, "the rule set and the context count the same transform types");

int xTransformFwdBatchDev(x266hip_ctx *ctx, int type, int size, const int16_t *d_in, int16_t *d_out, size_t n,
                          const uint32_t *d_offsets, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_batch(type, size, d_in, d_out, n, d_offsets)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    if (size == 32 && !d_offsets) return launch_op(ctx, 0, d_in, d_out, n, (hipStream_t)stream);
    const int l = size == 4 ? 0 : (size == 8 ? 1 : 2);
    LaunchCfg cfg = cfg_for(ctx, 0);
    cfg.units_per_wave = 1;                                             // one 32x32 tile per wave (profiles/r01_launch_sweep.txt)
    return launched(ctx, "transform launch", size == 32 ? launch_transform_small(5, d_in, d_out, n, ctx->d_fwd, d_offsets, cfg, (hipStream_t)stream)
                                                        : launch_transform_small(l + 2, d_in, d_out, n, ctx->d_tr[type][l], d_offsets, cfg, (hipStream_t)stream));
}

// All or nothing: the device tables are built from `next`, a COPY of the slot matrices with the wanted changes, and the context's
// own copy changes only once every upload has succeeded; after a failed upload the old tables are put back, and if even that fails
// the transform set of this context is marked unusable (its calls then fail) rather than left half old, half new.
static int commit_slot_matrices(x266hip_ctx *ctx, const SlotMatrices &next, const char *who)
{
    if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, X266HIP_EDEVICE, "transform matrices: device synchronisation");   // launches in flight read the tables
    DctOps *h = new (std::nothrow) DctOps;
    if (!h) return fail(ctx, X266HIP_ENOMEM, who);
    bool ok = true, touched = false;
    for (int slot = 0; slot < 2 && ok; ++slot)
        for (int l = 0; l < 3 && ok; ++l)
            if (std::memcmp(next[slot][l], ctx->slot_mat[slot][l], 256)) { touched = true; ok = upload_slot_tables(ctx, next, slot, l, h); }
    if (!ok) {
        bool back = true;
        for (int slot = 0; slot < 2 && back; ++slot)
            for (int l = 0; l < 3 && back; ++l)
                if (std::memcmp(next[slot][l], ctx->slot_mat[slot][l], 256)) back = upload_slot_tables(ctx, ctx->slot_mat, slot, l, h);
        ctx->tr_tables_valid = back;
    }
    delete h;
    if (!ok) return fail(ctx, X266HIP_EDEVICE, ctx->tr_tables_valid ? "transform matrices: table upload failed, previous matrices kept"
                                                                      : "transform matrices: table upload failed and the previous tables could not be restored: transform set unusable");
    if (touched) std::memcpy(ctx->slot_mat, next, sizeof(SlotMatrices));
    ctx->tr_tables_valid = true;
    return X266HIP_OK;
}

int xTransformSetMatrix(x266hip_ctx *ctx, int slot, int size, const int8_t *m)
{
    if (!ctx) return X266HIP_EINVAL;
    if (slot < 0 || slot > 1) return fail(ctx, X266HIP_EINVAL, "xTransformSetMatrix: slot must be 0 or 1");
    if (size != 4 && size != 8 && size != 16)
        return fail(ctx, X266HIP_EINVAL, "xTransformSetMatrix: size must be 4, 8 or 16 (the 32-point DCT-II is the reference's g_t32 and stays)");
    X_DEV(ctx);
    const int l = size == 4 ? 0 : (size == 8 ? 1 : 2);
    SlotMatrices next;
    std::memcpy(next, ctx->slot_mat, sizeof next);
    if (m) std::memcpy(next[slot][l], m, (size_t)size * size);
    else default_slot_matrix(slot, size, next[slot][l]);
    const int rc = commit_slot_matrices(ctx, next, "xTransformSetMatrix");
    if (rc == X266HIP_OK && slot == 1) ctx->slot1_preset = -1;
    return rc;
}

int xTransformUsePreset(x266hip_ctx *ctx, int preset)
{
    if (!ctx) return X266HIP_EINVAL;
    if (preset < X266_PRESET_CLOSED_FORM || preset > X266_PRESET_VTM_DCT8) return fail(ctx, X266HIP_EINVAL, "xTransformUsePreset: unknown preset");
    X_DEV(ctx);
    SlotMatrices next;
    std::memcpy(next, ctx->slot_mat, sizeof next);
    for (int l = 0; l < 3; ++l) {
        std::memset(next[1][l], 0, 256);
        if (preset == X266_PRESET_CLOSED_FORM) default_slot_matrix(1, 4 << l, next[1][l]);
        else vtm_slot1_matrix(4 << l, preset == X266_PRESET_VTM_DCT8, next[1][l]);
    }
    const int rc = commit_slot_matrices(ctx, next, "xTransformUsePreset");
    if (rc == X266HIP_OK) ctx->slot1_preset = preset;
    return rc;
}

int xTransformPreset(const x266hip_ctx *ctx) { return ctx ? ctx->slot1_preset : -1; }

int xTransformGetMatrix(const x266hip_ctx *ctx, int slot, int size, int8_t *m)
{
    if (!ctx || !m || slot < 0 || slot > 1 || (size != 4 && size != 8 && size != 16)) return X266HIP_EINVAL;
    std::memcpy(m, ctx->slot_mat[slot][size == 4 ? 0 : (size == 8 ? 1 : 2)], (size_t)size * size);
    return X266HIP_OK;
}

int xTransformTilesDev(x266hip_ctx *ctx, int inverse, const int16_t *d_in, int16_t *d_out, size_t n_tiles,
                       const uint32_t *d_tile_offsets, const uint8_t *d_tile_class, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_tiles(d_in, d_out, n_tiles, d_tile_offsets, d_tile_class)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    LaunchCfg cfg = cfg_for(ctx, inverse ? 1 : 0);
    cfg.lds_bytes_per_wave = x266hip_ctx::kTileLdsPerWave;
    cfg.units_per_wave = ctx->tile_tiles_per_wave ? ctx->tile_tiles_per_wave : 2;   // measured optimum (profiles/r03_tiles_one_launch.txt): the wave's table copy serves two tiles
    return launched(ctx, "tile transform launch", launch_transform_tiles(inverse != 0, d_in, d_out, n_tiles, d_tile_offsets, d_tile_class,
                                                                         inverse ? ctx->d_tile_inv : ctx->d_tile_fwd, cfg, (hipStream_t)stream));
}

int xConvInputFmtDev(x266hip_ctx *ctx, x266_ref_block_t *d_tiles, const uint8_t *d_y, const uint8_t *d_u, const uint8_t *d_v,
                     intptr_t strdY, int width, int height, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::tile_convert(true, d_tiles, d_y, d_u, d_v, strdY, 0, width, height)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "tile pack launch", launch_tile_convert(true, d_tiles, const_cast<uint8_t *>(d_y), const_cast<uint8_t *>(d_u), const_cast<uint8_t *>(d_v),
                                                                 (long long)strdY, (long long)(strdY >> 1), width, height, (hipStream_t)stream));
}

int xConvOutput420Dev(x266hip_ctx *ctx, const x266_ref_block_t *d_tiles, uint8_t *d_y, intptr_t strdY, uint8_t *d_u, uint8_t *d_v,
                      intptr_t strdC, int width, int height, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::tile_convert(false, d_tiles, d_y, d_u, d_v, strdY, strdC, width, height)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "tile unpack launch", launch_tile_convert(false, const_cast<x266_ref_block_t *>(d_tiles), d_y, d_u, d_v, (long long)strdY, (long long)strdC,
                                                                   width, height, (hipStream_t)stream));
}

int xResidualLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                     int block_edge, int16_t *d_residual, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::residual_luma(d_cur, d_pred, width, height, block_edge, d_residual)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "residual launch", launch_residual_luma(block_edge, d_cur, d_pred, d_residual, width, height, (hipStream_t)stream));
}

int xDct32FwdFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                          int16_t *d_coef, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::from_tiles(d_cur, d_pred, width, height, 32, d_coef, 16)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused transform launch", launch_dct32_from_tiles(d_cur, d_pred, d_coef, width, height, ctx->d_fwd, cfg_for(ctx, 0), (hipStream_t)stream));
}

int xSatd8x8FromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                         uint32_t *d_out, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::from_tiles(d_cur, d_pred, width, height, 16, d_out, 4)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused satd launch", launch_satd8x8_from_tiles(d_cur, d_pred, d_out, width, height,
                                                                        ctx->satd_variant == 1 || ctx->satd_variant == 3 ? ctx->satd_variant : 0, (hipStream_t)stream));
}

int xResidualChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                       int block_edge, int16_t *d_res_u, int16_t *d_res_v, size_t block_pitch, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::chroma_from_tiles(d_cur, d_pred, width, height, block_edge, d_res_u, d_res_v, 16, (size_t)block_edge * block_edge * 2, block_pitch))
        return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "chroma residual launch", launch_residual_chroma(block_edge, d_cur, d_pred, d_res_u, d_res_v, block_pitch, width, height, (hipStream_t)stream));
}

int xDct32FwdChromaFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                                int16_t *d_coef_u, int16_t *d_coef_v, size_t block_pitch, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::chroma_from_tiles(d_cur, d_pred, width, height, 32, d_coef_u, d_coef_v, 16, 2048, block_pitch)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused chroma transform launch",
                    launch_dct32_chroma_from_tiles(d_cur, d_pred, d_coef_u, d_coef_v, block_pitch, width, height, ctx->d_fwd, cfg_for(ctx, 0), (hipStream_t)stream));
}

int xDct32FwdCtuFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                             int16_t *d_coef, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::from_tiles(d_cur, d_pred, width, height, 64, d_coef, 16)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused CTU transform launch", launch_dct32_ctu_from_tiles(d_cur, d_pred, d_coef, width, height, ctx->d_fwd, cfg_for(ctx, 0), (hipStream_t)stream));
}

// ---- reconstruction into tiles: the way back from residuals / coefficients to a frame --------------------------------------
int xReconLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_pred, const int16_t *d_residual, int width, int height,
                  int block_edge, x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::recon_luma(d_pred, d_residual, width, height, block_edge, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "recon launch", launch_recon_luma(block_edge, d_pred, d_residual, d_recon, width, height, (hipStream_t)stream));
}

int xReconChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_pred, const int16_t *d_res_u, const int16_t *d_res_v, size_t block_pitch,
                    int width, int height, int block_edge, x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::recon_chroma(d_pred, d_res_u, d_res_v, block_pitch, width, height, block_edge, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "chroma recon launch", launch_recon_chroma(block_edge, d_pred, d_res_u, d_res_v, block_pitch, d_recon, width, height, (hipStream_t)stream));
}

static LaunchCfg inv_to_tiles_cfg(const x266hip_ctx *ctx)
{
    LaunchCfg cfg = cfg_for(ctx, 1);
    cfg.lds_bytes_per_wave = x266hip_ctx::kDctInvLdsPerWave;
    return cfg;
}

int xDct32InvToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const x266_ref_block_t *d_pred, int width, int height,
                        x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::inv_to_tiles(d_coef, d_pred, width, height, 32, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused inverse transform launch",
                    launch_dct32_inv_to_tiles(d_coef, d_pred, d_recon, width, height, ctx->d_inv_lds, inv_to_tiles_cfg(ctx), (hipStream_t)stream));
}

int xDct32InvCtuToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const x266_ref_block_t *d_pred, int width, int height,
                           x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::inv_to_tiles(d_coef, d_pred, width, height, 64, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused CTU inverse launch",
                    launch_dct32_inv_ctu_to_tiles(d_coef, d_pred, d_recon, width, height, ctx->d_inv_lds, inv_to_tiles_cfg(ctx), (hipStream_t)stream));
}

// ---- the mixed transform set from and into tiles, per CTU ----------------------------------------------------------------------
static LaunchCfg ctu_tiles_cfg(const x266hip_ctx *ctx, int inverse)
{
    LaunchCfg cfg = cfg_for(ctx, inverse);
    cfg.lds_bytes_per_wave = x266hip_ctx::kTileLdsPerWave;
    return cfg;
}

int xTransformCtuFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                              const uint8_t *d_class, int16_t *d_coef, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_ctu_from_tiles(d_cur, d_pred, width, height, d_class, d_coef)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    return launched(ctx, "CTU transform from tiles launch", launch_transform_ctu_tiles(false, d_cur, nullptr, d_pred, d_class, d_coef, nullptr, width, height, ctx->d_tile_fwd,
                                                                                       ctu_tiles_cfg(ctx, 0), (hipStream_t)stream));
}

int xTransformCtuToTilesDev(x266hip_ctx *ctx, const int16_t *d_coef, const uint8_t *d_class, const x266_ref_block_t *d_pred, int width,
                            int height, x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_ctu_to_tiles(d_coef, d_class, d_pred, width, height, d_recon)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    return launched(ctx, "CTU transform into tiles launch", launch_transform_ctu_tiles(true, nullptr, d_coef, d_pred, d_class, nullptr, d_recon, width, height, ctx->d_tile_inv,
                                                                                       ctu_tiles_cfg(ctx, 1), (hipStream_t)stream));
}

// ---- the quantiser (x266_quant.hpp) -----------------------------------------------------------------------------------------------
int xQuantRegionsGpu(x266hip_ctx *ctx, int inverse, const int16_t *d_in, int16_t *d_out, size_t n_regions, const uint8_t *d_class,
                     const uint8_t *d_qp, int qp, int rounding, uint32_t *d_nnz, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::quant_regions(inverse, d_in, d_out, n_regions, d_class, d_qp, qp, rounding, d_nnz)) return refuse(ctx, __func__, why);
    if (n_regions == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "quantiser launch", launch_quant_regions(inverse != 0, d_in, d_out, n_regions, d_class, d_qp, qp, rounding, d_nnz, (hipStream_t)stream));
}

int xDct32CodeCtuTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                          const uint8_t *d_qp, int qp, int rounding, int16_t *d_level, uint32_t *d_nnz, x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::dct32_code_ctu_tiles(d_cur, d_pred, width, height, d_qp, qp, rounding, d_level, d_nnz, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused CTU coding launch", launch_dct32_code_ctu_tiles(d_cur, d_pred, d_recon, d_level, d_nnz, d_qp, qp, rounding, width, height, ctx->d_fwd,
                                                                               ctx->d_inv_acc, inv_to_tiles_cfg(ctx), (hipStream_t)stream));
}

int xSatd8x8ChromaFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_pred, int width, int height,
                               uint32_t *d_out_u, uint32_t *d_out_v, size_t pitch, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::chroma_from_tiles(d_cur, d_pred, width, height, 8, d_out_u, d_out_v, 4, 4, pitch)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "fused chroma satd launch", launch_satd8x8_chroma_from_tiles(d_cur, d_pred, d_out_u, d_out_v, pitch, width, height, (hipStream_t)stream));
}

int xSadBatchDev(x266hip_ctx *ctx, int edge, const uint8_t *d_a, const uint8_t *d_b, uint32_t *d_out, size_t n, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::sad_batch(edge, d_a, d_b, d_out, n)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    hipError_t e;
    const size_t in_bytes = n * (size_t)(edge * edge);
    if (ctx->autotune && n && edge >= 8 && !ranges_overlap(d_a, in_bytes, d_out, n * 4) && !ranges_overlap(d_b, in_bytes, d_out, n * 4)) {
        auto run = [&](int c) { return launch_sad(edge, d_a, d_b, d_out, n, kSadCands[c].wg_threads / 64, kSadCands[c].lds_bytes_per_wave, (hipStream_t)stream); };
        const int family = edge == 8 ? x266hip_ctx::kTuneSad8 : edge == 16 ? x266hip_ctx::kTuneSad16 : edge == 32 ? x266hip_ctx::kTuneSad32 : x266hip_ctx::kTuneSad64;
        if (const int rc = run_family(ctx, __func__, family, (int)(sizeof kSadCands / sizeof kSadCands[0]), in_bytes >= ((size_t)128 << 20), (hipStream_t)stream, run, &e)) return rc;
    } else {
        e = launch_sad(edge, d_a, d_b, d_out, n, 0, 0, (hipStream_t)stream);
    }
    return launched(ctx, "sad launch", e);
}

int xTransformInvBatchDev(x266hip_ctx *ctx, int type, int size, const int16_t *d_in, int16_t *d_out, size_t n,
                          const uint32_t *d_offsets, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_batch(type, size, d_in, d_out, n, d_offsets)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    if (size == 32 && !d_offsets) return launch_op(ctx, 1, d_in, d_out, n, (hipStream_t)stream);
    const int l = size == 4 ? 0 : (size == 8 ? 1 : 2);
    const LaunchCfg cfg = cfg_for(ctx, 1);
    return launched(ctx, "inverse transform launch", size == 32 ? launch_transform_small_inv(5, d_in, d_out, n, ctx->d_inv_lds, d_offsets, cfg, (hipStream_t)stream)
                                                                : launch_transform_small_inv(l + 2, d_in, d_out, n, ctx->d_tr_inv[type][l], d_offsets, cfg, (hipStream_t)stream));
}

int xHipMeScratchReserve(x266hip_ctx *ctx, void *stream, int width, int height)
{
    if (!ctx) return X266HIP_EINVAL;
    if (width < 8 || height < 8) return fail(ctx, X266HIP_EINVAL, "xHipMeScratchReserve: frame size");
    X_DEV(ctx);
    x266hip_ctx::MeScratch *slot = nullptr;
    return me_scratch_for(ctx, (hipStream_t)stream, width, height, &slot);
}

// ---- motion search and compensation ---------------------------------------------------------------------------------------------
// The SATD searches keep their transformed current frame in the stream's scratch; planar = strides given, else frames of tiles.
static int satd_search_call(x266hip_ctx *ctx, bool tiles, const uint8_t *d_cur, intptr_t cur_stride, const uint8_t *d_ref, intptr_t ref_stride, int width, int height,
                            int range, x266_me_result_t *d_best, uint32_t *d_costs, void *stream)
{
    X_DEV(ctx);
    x266hip_ctx::MeScratch *slot = nullptr;
    if (const int rc = me_scratch_for(ctx, (hipStream_t)stream, width, height, &slot)) return rc;
    (void)hipGetLastError();
    const hipError_t e = launch_satd_search(d_cur, (long long)cur_stride, d_ref, (long long)ref_stride, width, height, range, d_best, d_costs, ctx->me_tile_rows, slot->p,
                                            ctx->prop.multiProcessorCount, tiles, (hipStream_t)stream);
    if (e == hipSuccess && slot->last_use && !slot->capturing_now) (void)hipEventRecord(slot->last_use, (hipStream_t)stream);   // what an eviction waits for
    return launched(ctx, "search launch", e);
}

int xSatd8x8SearchDev(x266hip_ctx *ctx, const uint8_t *d_cur, intptr_t cur_stride, const uint8_t *d_ref,
                      intptr_t ref_stride, int width, int height, int range, x266_me_result_t *d_best,
                      uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::plane_search(false, d_cur, cur_stride, d_ref, ref_stride, width, height, range, d_best, d_costs)) return refuse(ctx, __func__, why);
    return satd_search_call(ctx, false, d_cur, cur_stride, d_ref, ref_stride, width, height, range, d_best, d_costs, stream);
}

int xSad8x8SearchDev(x266hip_ctx *ctx, const uint8_t *d_cur, intptr_t cur_stride, const uint8_t *d_ref,
                     intptr_t ref_stride, int width, int height, int range, x266_me_result_t *d_best,
                     uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::plane_search(true, d_cur, cur_stride, d_ref, ref_stride, width, height, range, d_best, d_costs)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "SAD search launch", launch_sad_search(d_cur, (long long)cur_stride, d_ref, (long long)ref_stride, width, height, range,
                                                                d_best, d_costs, ctx->me_tile_rows, false, (hipStream_t)stream));
}

int xSatd8x8SearchFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref, int width, int height,
                               int range, x266_me_result_t *d_best, uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::tile_search(d_cur, d_ref, width, height, range, d_best, d_costs)) return refuse(ctx, __func__, why);
    return satd_search_call(ctx, true, reinterpret_cast<const uint8_t *>(d_cur), 0, reinterpret_cast<const uint8_t *>(d_ref), 0, width, height, range, d_best, d_costs, stream);
}

int xSad8x8SearchFromTilesDev(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref, int width, int height,
                              int range, x266_me_result_t *d_best, uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::tile_search(d_cur, d_ref, width, height, range, d_best, d_costs)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "SAD search launch", launch_sad_search(reinterpret_cast<const uint8_t *>(d_cur), 0, reinterpret_cast<const uint8_t *>(d_ref), 0, width, height,
                                                                range, d_best, d_costs, ctx->me_tile_rows, true, (hipStream_t)stream));
}

// The six motion compensation calls share their argument rules and differ in the planes they write; the quarter-sample ones
// (qpel) also hold every span against the end of the address space.
typedef hipError_t (*mc_launch_fn)(const x266_ref_block_t *, const x266_me_result_t *, x266_ref_block_t *, int, int, hipStream_t);

static int motion_comp_call(x266hip_ctx *ctx, const char *name, bool qpel, mc_launch_fn launch, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv,
                            int width, int height, x266_ref_block_t *d_pred, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::motion_comp(qpel, d_ref, d_mv, width, height, d_pred)) return refuse(ctx, name, why);
    X_DEV(ctx);
    return launched(ctx, qpel ? "quarter-sample motion compensation launch" : "motion compensation launch", launch(d_ref, d_mv, d_pred, width, height, (hipStream_t)stream));
}

int xMotionCompLumaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                       x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, false, launch_motion_comp_luma, d_ref, d_mv, width, height, d_pred, stream);
}

int xMotionCompChromaDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                         x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, false, launch_motion_comp_chroma, d_ref, d_mv, width, height, d_pred, stream);
}

int xMotionCompDev(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                   x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, false, launch_motion_comp, d_ref, d_mv, width, height, d_pred, stream);
}

int xMotionCompQpelLumaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                           x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, true, launch_mc_qpel_luma, d_ref, d_mv, width, height, d_pred, stream);
}

int xMotionCompQpelChromaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                             x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, true, launch_mc_qpel_chroma, d_ref, d_mv, width, height, d_pred, stream);
}

int xMotionCompQpelGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_ref, const x266_me_result_t *d_mv, int width, int height,
                       x266_ref_block_t *d_pred, void *stream)
{
    return motion_comp_call(ctx, __func__, true, launch_mc_qpel, d_ref, d_mv, width, height, d_pred, stream);
}

int xSatd8x8RefineQpelFromTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref, int width, int height,
                                   const x266_me_result_t *d_int, x266_me_result_t *d_best, uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::refine_qpel(d_cur, d_ref, width, height, d_int, d_best, d_costs)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "quarter-sample refinement launch", launch_satd_refine_qpel(d_cur, d_ref, width, height, d_int, d_best, d_costs, (hipStream_t)stream));
}

// The bi-directional calls: wp is read here, on the host, and travels by value into the launch; NULL is w = 1, o = 0, log2_denom = 0,
// which IS the default formula.
static x266_wp_t wp_or_default(const x266_wp_t *wp)
{
    const x266_wp_t unit = {{{1, 1, 1}, {1, 1, 1}}, {{0, 0, 0}, {0, 0, 0}}, {0, 0}};
    return wp ? *wp : unit;
}

int xMotionCompBiQpelTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, const x266_me_result_t *d_mv0,
                           const x266_me_result_t *d_mv1, const uint8_t *d_dir, const x266_wp_t *wp, int planes, int width, int height,
                           x266_ref_block_t *d_pred, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::mc_bi_qpel(d_ref0, d_ref1, d_mv0, d_mv1, d_dir, wp, planes, width, height, d_pred)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "bi-directional motion compensation launch",
                    launch_mc_bi_qpel(planes, d_ref0, d_ref1, d_mv0, d_mv1, d_dir, wp_or_default(wp), d_pred, width, height, (hipStream_t)stream));
}

int xSatd8x8BiCostsFromTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref0, const x266_ref_block_t *d_ref1, int width,
                             int height, const x266_me_result_t *d_mv0, const x266_me_result_t *d_mv1, const x266_wp_t *wp, int bi_penalty,
                             uint32_t *d_costs, uint8_t *d_dir, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::bi_costs(d_cur, d_ref0, d_ref1, width, height, d_mv0, d_mv1, wp, bi_penalty, d_costs, d_dir)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "bi-directional cost launch",
                    launch_satd_bi_costs(d_cur, d_ref0, d_ref1, width, height, d_mv0, d_mv1, wp_or_default(wp), bi_penalty, d_costs, d_dir, (hipStream_t)stream));
}

int xSatd8x8RefineBiQpelFromTiles(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, const x266_ref_block_t *d_ref_fix, const x266_me_result_t *d_mv_fix,
                                  const x266_ref_block_t *d_ref, const x266_me_result_t *d_int, int list, const x266_wp_t *wp, int width, int height,
                                  x266_me_result_t *d_best, uint32_t *d_costs, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::refine_bi_qpel(d_cur, d_ref_fix, d_mv_fix, d_ref, d_int, list, wp, width, height, d_best, d_costs)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "bi-directional refinement launch",
                    launch_satd_refine_bi_qpel(d_cur, d_ref_fix, d_mv_fix, d_ref, d_int, list, wp_or_default(wp), width, height, d_best, d_costs, (hipStream_t)stream));
}

// ---- in-loop deblocking of tiled frames (x266_deblock.hpp) ---------------------------------------------------------------------------
// The three calls share their argument rules and differ in the planes they write (1 = m_Y, 2 = m_C, 3 = both).
static int deblock_call(x266hip_ctx *ctx, const char *name, int planes, const x266_ref_block_t *d_in, int width, int height,
                        const x266_deblock_t *p, x266_ref_block_t *d_out, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::deblock(d_in, width, height, p, d_out)) return refuse(ctx, name, why);
    X_DEV(ctx);
    return launched(ctx, "deblocking launch", launch_deblock(planes, d_in, d_out, width, height, *p, (hipStream_t)stream));
}

int xDeblockLumaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p, x266_ref_block_t *d_out,
                    void *stream)
{
    return deblock_call(ctx, __func__, 1, d_in, width, height, p, d_out, stream);
}

int xDeblockChromaGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p, x266_ref_block_t *d_out,
                      void *stream)
{
    return deblock_call(ctx, __func__, 2, d_in, width, height, p, d_out, stream);
}

int xDeblockGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_deblock_t *p, x266_ref_block_t *d_out,
                void *stream)
{
    return deblock_call(ctx, __func__, 3, d_in, width, height, p, d_out, stream);
}

// ---- sample adaptive offset on tiled frames (x266_sao.hpp) -----------------------------------------------------------------------------
static int sao_stats_call(x266hip_ctx *ctx, const char *name, bool decide, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width,
                          int height, int lambda_q4, x266_sao_t *d_param, int32_t *d_stats, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::sao_stats(decide, d_org, d_dec, width, height, lambda_q4, d_param, d_stats)) return refuse(ctx, name, why);
    X_DEV(ctx);
    return launched(ctx, "SAO statistics launch", launch_sao_stats(d_org, d_dec, width, height, lambda_q4, d_stats, d_param, (hipStream_t)stream));
}

int xSaoStatsGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, int32_t *d_stats, void *stream)
{
    return sao_stats_call(ctx, __func__, false, d_org, d_dec, width, height, 0, nullptr, d_stats, stream);
}

int xSaoSearchGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, int lambda_q4,
                  x266_sao_t *d_param, int32_t *d_stats, void *stream)
{
    return sao_stats_call(ctx, __func__, true, d_org, d_dec, width, height, lambda_q4, d_param, d_stats, stream);
}

int xSaoDecideGpu(x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, int lambda_q4, x266_sao_t *d_param, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::sao_decide(d_stats, n_ctu, lambda_q4, d_param)) return refuse(ctx, __func__, why);
    if (n_ctu == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "SAO decision launch", launch_sao_decide(d_stats, n_ctu, lambda_q4, d_param, (hipStream_t)stream));
}

int xSaoApplyGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const x266_sao_t *d_param, x266_ref_block_t *d_out,
                 void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::sao_apply(d_in, width, height, d_param, d_out)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "SAO apply launch", launch_sao_apply(d_in, d_out, width, height, d_param, (hipStream_t)stream));
}

// ---- adaptive loop filter on tiled frames (x266_alf.hpp) -------------------------------------------------------------------------------
int xAlfClassifyGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_dec, int width, int height, uint8_t *d_class, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::alf_classify(d_dec, width, height, d_class)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "ALF classification launch", launch_alf_classify(d_dec, width, height, d_class, (hipStream_t)stream));
}

int xAlfStatsGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_org, const x266_ref_block_t *d_dec, int width, int height, const uint8_t *d_class,
                 int32_t *d_stats, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::alf_stats(d_org, d_dec, width, height, d_class, d_stats)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "ALF statistics launch", launch_alf_stats(d_org, d_dec, width, height, d_class, d_stats, (hipStream_t)stream));
}

int xAlfSumStatsGpu(x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, const uint8_t *d_mask, int64_t *d_total, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::alf_sum_stats(d_stats, n_ctu, d_mask, d_total)) return refuse(ctx, __func__, why);
    if (n_ctu == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "ALF totals launch", launch_alf_sum_stats(d_stats, n_ctu, d_mask, d_total, (hipStream_t)stream));
}

int xAlfDecideGpu(x266hip_ctx *ctx, const int32_t *d_stats, size_t n_ctu, const x266_alf_luma_t *d_luma, int n_luma, const x266_alf_chroma_t *d_chroma,
                  int n_chroma, int lambda_q4, uint8_t *d_ctrl, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::alf_decide(d_stats, n_ctu, d_luma, n_luma, d_chroma, n_chroma, lambda_q4, d_ctrl)) return refuse(ctx, __func__, why);
    if (n_ctu == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "ALF decision launch", launch_alf_decide(d_stats, n_ctu, d_luma, n_luma, d_chroma, n_chroma, lambda_q4, d_ctrl, (hipStream_t)stream));
}

int xAlfApplyGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_in, int width, int height, const uint8_t *d_class, const x266_alf_luma_t *d_luma, int n_luma,
                 const x266_alf_chroma_t *d_chroma, int n_chroma, const uint8_t *d_ctrl, x266_ref_block_t *d_out, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::alf_apply(d_in, width, height, d_class, d_luma, n_luma, d_chroma, n_chroma, d_ctrl, d_out)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "ALF apply launch", launch_alf_apply(d_in, d_out, width, height, d_class, d_luma, n_luma, d_chroma, n_chroma, d_ctrl, (hipStream_t)stream));
}

// ---- intra coding of tiled frames (intra_frame_kernels.hip) ------------------------------------------------------------------------------
int xIntra32RefsFromTilesGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_frame, int width, int height, int component, x266_intra_ref_t *d_refs,
                             void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::intra32_refs_from_tiles(d_frame, width, height, component, d_refs)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "intra reference gather launch", launch_intra32_refs_from_tiles(d_frame, width, height, component, d_refs, (hipStream_t)stream));
}

int xIntra32CodeFrameGpu(x266hip_ctx *ctx, const x266_ref_block_t *d_cur, int width, int height, const uint8_t *d_qp, int qp, int rounding,
                         const uint8_t *d_mode_in, int16_t *d_level, uint32_t *d_nnz, uint8_t *d_mode, x266_ref_block_t *d_recon, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::intra32_code_frame(d_cur, width, height, d_qp, qp, rounding, d_mode_in, d_level, d_nnz, d_mode, d_recon)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "intra frame coding launch", launch_intra32_code_frame(d_cur, d_recon, d_level, d_nnz, d_qp, qp, rounding, d_mode_in, d_mode, width, height, ctx->d_fwd,
                                                                               ctx->d_inv_acc, (hipStream_t)stream));
}

int xDct32CodeMixedFrameGpu(x266hip_ctx *ctx, const x266_mixed_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::mixed_code_frame(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "mixed frame coding launch", launch_mixed_code_frame(*p, ctx->d_fwd, ctx->d_inv_acc, (hipStream_t)stream));
}

// ---- the compact level stream (levels_kernels.hip, x266_levels.hpp) ------------------------------------------------------------------------
int xLevelsPackGpu(x266hip_ctx *ctx, const x266_levels_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::levels_pack(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "level pack launch", launch_levels_pack(*p, (hipStream_t)stream));
}

int xLevelsUnpackGpu(x266hip_ctx *ctx, const x266_levels_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::levels_unpack(p)) return refuse(ctx, __func__, why);
    if (p->n_regions == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "level unpack launch", launch_levels_unpack(*p, (hipStream_t)stream));
}

int xLevelScan(int size, uint16_t *pos)
{
    if (!pos || (size != 4 && size != 8 && size != 16 && size != 32)) return X266HIP_EINVAL;
    const unsigned n = (unsigned)size, k = size == 4 ? 0u : size == 8 ? 1u : size == 16 ? 2u : 3u;
    for (unsigned s = 0; s < n * n / 16; ++s)                               // block 0 of a region of this class: CG bit s is scan position s
        for (unsigned i = 0; i < 16; ++i) pos[s * 16 + i] = (uint16_t)(level_cg_origin(k, s) + (level_scan4(i) >> 2) * n + (level_scan4(i) & 3u));
    return X266HIP_OK;
}

unsigned xLevelsScanChunk(void) { return levels_scan_chunk(); }

// ---- RDOQ and the level rate estimate (rdoq_kernels.hip, x266_rdoq.hpp) --------------------------------------------------------------------
int xRdoQuantRegionsGpu(x266hip_ctx *ctx, const x266_rdoq_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::rdoq_regions(p)) return refuse(ctx, __func__, why);
    if (p->n_regions == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "RDOQ launch", launch_rdo_quant_regions(*p, (hipStream_t)stream));
}

int xLevelsBitsGpu(x266hip_ctx *ctx, const x266_rdoq_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::levels_bits(p)) return refuse(ctx, __func__, why);
    if (p->n_regions == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "level rate launch", launch_levels_bits(*p, (hipStream_t)stream));
}

// the transform decision: the forward tables of the mixed set, like xTransformCtuFromTilesDev
int xTransformDecideCtuTilesGpu(x266hip_ctx *ctx, const x266_tdecide_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::transform_decide(p)) return refuse(ctx, __func__, why);
    if (!ctx->tr_tables_valid) return tables_invalid(ctx, __func__);
    X_DEV(ctx);
    return launched(ctx, "transform decision launch", launch_transform_decide(*p, ctx->d_tile_fwd, (hipStream_t)stream));
}

int xLevelBits(int abs_level, int pos_class)
{
    if (abs_level < 0 || abs_level > 32768 || pos_class < 0 || pos_class > 2) return -1;
    return (int)rdoq_level_bits((unsigned)abs_level, rdoq_sig_bits((unsigned)pos_class, 0), rdoq_sig_bits((unsigned)pos_class, 1));
}

int xLastPosBits(int u, int v, int log2_size)
{
    if (log2_size < 2 || log2_size > 5 || u < 0 || v < 0 || u >= (1 << log2_size) || v >= (1 << log2_size)) return -1;
    return (int)(16u * (rdoq_last_pos((unsigned)u, (unsigned)log2_size) + rdoq_last_pos((unsigned)v, (unsigned)log2_size)));
}

int xCgFlagBits(int coded) { return coded == 0 || coded == 1 ? (int)rdoq_cg_flag_bits((unsigned)coded) : -1; }

// ---- source analysis (aq_kernels.hip, x266_aq.hpp) ---------------------------------------------------------------------------------------------
int xAqStatsGpu(x266hip_ctx *ctx, const x266_aq_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::aq_stats(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "source statistics launch", launch_aq_stats(*p, (hipStream_t)stream));
}

int xAqDecideGpu(x266hip_ctx *ctx, const x266_aq_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::aq_decide(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "qp map launch", launch_aq_decide(*p, (hipStream_t)stream));
}

int xAqTotalsChunk(void) { return aq_totals_chunk(); }

int xWeightsFromTotals(const int64_t cur[8], const int64_t ref[8], int list, x266_wp_t *wp)
{
    if (args::weights_from_totals(cur, ref, list, wp)) return X266HIP_EINVAL;
    for (int plane = 0; plane < 3; ++plane) aq_plane_weight(cur, ref, plane, wp->log2_denom[plane ? 1 : 0], &wp->w[list][plane], &wp->o[list][plane]);
    return X266HIP_OK;
}

// ---- frame quality (quality_kernels.hip, x266_quality.hpp) --------------------------------------------------------------------------------------
int xQualityStatsGpu(x266hip_ctx *ctx, const x266_quality_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::quality_stats(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "frame quality launch", launch_quality_stats(*p, (hipStream_t)stream));
}

int xQualityTotalsChunk(void) { return quality_totals_chunk(); }

int xQualityFromTotals(const int64_t total[8], int width, int height, double psnr[4], double ssim[3])
{
    if (args::quality_from_totals(total, width, height, psnr, ssim)) return X266HIP_EINVAL;
    quality_from_totals(total, width, height, psnr, ssim);
    return X266HIP_OK;
}

// ---- the lookahead (lookahead_kernels.hip, x266_lookahead.hpp) -----------------------------------------------------------------------------------
int xLaDownscaleGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::la_downscale(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "lowres frame launch", launch_la_downscale(*p, (hipStream_t)stream));
}

int xLaIntraCostsGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::la_intra_costs(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "lowres intra cost launch", launch_la_intra_costs(*p, (hipStream_t)stream));
}

int xLaFrameCostGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::la_frame_cost(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "frame cost launch", launch_la_frame_cost(*p, (hipStream_t)stream));
}

int xLaPropagateGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::la_propagate(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "propagation launch", launch_la_propagate(*p, (hipStream_t)stream));
}

int xLaTreeQpGpu(x266hip_ctx *ctx, const x266_la_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::la_tree_qp(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "tree qp launch", launch_la_tree_qp(*p, (hipStream_t)stream));
}

int xLaTotalsChunk(void) { return la_totals_chunk(); }

int xSceneCutFromTotals(const int64_t total[8], int threshold_q8, int frames_since_key, int min_keyint, int max_keyint)
{
    if (args::scene_cut_from_totals(total, threshold_q8, frames_since_key, min_keyint, max_keyint)) return X266HIP_EINVAL;
    return la_scene_cut(total, threshold_q8, frames_since_key, min_keyint, max_keyint);
}

// ---- the seeded search (seeded_search_kernels.hip, x266_seed.hpp) ----------------------------------------------------------------------------------
int xSatd8x8SeededSearchGpu(x266hip_ctx *ctx, const x266_seed_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::seeded_search(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "seeded search launch", launch_seeded_search(*p, (hipStream_t)stream));
}

// ---- the inter partition decision (partition_kernels.hip, x266_part.hpp) ---------------------------------------------------------------------------
int xInterPartitionDecideGpu(x266hip_ctx *ctx, const x266_part_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::partition_decide(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "partition decision launch", launch_partition_decide(*p, (hipStream_t)stream));
}

// ---- the compact motion stream (motion_kernels.hip, x266_motion.hpp) -------------------------------------------------------------------------------
int xMotionPackGpu(x266hip_ctx *ctx, const x266_motion_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::motion_pack(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "motion pack launch", launch_motion_pack(*p, (hipStream_t)stream));
}

int xMotionUnpackGpu(x266hip_ctx *ctx, const x266_motion_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::motion_unpack(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "motion unpack launch", launch_motion_unpack(*p, (hipStream_t)stream));
}

// the three host helpers: the functions of x266_motion.hpp that the kernels run, on the host
int xMotionWalk(int width, int height, size_t ctu, uint64_t head_mask, uint8_t head[64], uint8_t level[64])
{
    if (args::frame(width, height, 16) || !head || !level || ctu >= args::ctus(width, height)) return X266HIP_EINVAL;
    const MotionCtu g = motion_ctu(width / 8, height / 8, ctu);
    if (!motion_mask_well_formed(g, head_mask)) return X266HIP_EINVAL;
    int parts = 0;
    for (unsigned i = 0; i < 64; ++i) {
        head[i] = level[i] = 0;
        if (head_mask >> i & 1u) {                                          // ascending Morton index is the coding order
            head[parts] = (uint8_t)i;
            level[parts++] = (uint8_t)motion_head_level(g, head_mask, i);
        }
    }
    return parts;
}

int xMotionPredictor(int width, int height, const x266_me_result_t *field, int X, int Y, int level, int16_t p[2])
{
    if (args::frame(width, height, 16) || !field || !p || level < 0 || level >= kPartLevels) return X266HIP_EINVAL;
    const int bw = width / 8, bh = height / 8, n = 1 << level;
    if (X < 0 || Y < 0 || (X & (n - 1)) || (Y & (n - 1)) || !part_whole(bw, bh, level, X >> level, Y >> level)) return X266HIP_EINVAL;
    const PartVec v = motion_predictor(field, bw, X, Y, n);
    p[0] = (int16_t)v.x;
    p[1] = (int16_t)v.y;
    return X266HIP_OK;
}

int xMotionVectorBits(int d) { return d < -kMotionMaxDiff || d > kMotionMaxDiff ? -1 : seed_code_length(d); }

// ---- the entropy coder of the level stream (entropy_kernels.hip, x266_entropy.hpp) -------------------------------------------------------------------
int xEntropyEncodeLevelsGpu(x266hip_ctx *ctx, const x266_entropy_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_encode(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "entropy encode launch", launch_entropy_encode(*p, (hipStream_t)stream));
}

int xEntropyDecodeLevelsGpu(x266hip_ctx *ctx, const x266_entropy_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_decode(p)) return refuse(ctx, __func__, why);
    if (p->n_regions == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "entropy decode launch", launch_entropy_decode(*p, (hipStream_t)stream));
}

// the three host helpers: the functions of x266_entropy.hpp that the kernels run, on the host
int xEntropyDefaultInit(uint16_t init[X266_ENTROPY_CONTEXTS])
{
    if (!init) return X266HIP_EINVAL;
    for (unsigned i = 0; i < kEntropyContexts; ++i) init[i] = kEntropyDefault.p[i];
    return X266HIP_OK;
}

int xEntropyEncodeRegion(const int16_t *level, int cls, const uint16_t *init, uint8_t *out, size_t cap, uint32_t bins[2])
{
    if (!level || (!out && cap) || !args::entropy_init_ok(init)) return X266HIP_EINVAL;
    const unsigned k = (unsigned)cls & 3u;
    uint16_t ctx[kEntropyCtxPerSize];
    for (unsigned i = 0; i < kEntropyCtxPerSize; ++i) ctx[i] = (init ? init : kEntropyDefault.p)[k * kEntropyCtxPerSize + i];
    EntropyEnc e;
    entropy_enc_start(e, out, cap > kEntropyMaxBytes ? kEntropyMaxBytes : (uint32_t)cap);
    entropy_encode_region(e, level, k, entropy_cg_mask(level, k), ctx);
    const uint32_t n_bytes = entropy_enc_finish(e);
    if (bins) {
        bins[0] = e.ctx_bins;
        bins[1] = e.bypass_bins;
    }
    return (int)n_bytes;
}

int xEntropyDecodeRegion(const uint8_t *bytes, size_t n_bytes, int cls, const uint16_t *init, int16_t *level, uint32_t *n_nz)
{
    if (!level || (!bytes && n_bytes) || n_bytes > kEntropyMaxBytes || !args::entropy_init_ok(init)) return X266HIP_EINVAL;
    const unsigned k = (unsigned)cls & 3u;
    uint16_t ctx[kEntropyCtxPerSize];
    for (unsigned i = 0; i < kEntropyCtxPerSize; ++i) ctx[i] = (init ? init : kEntropyDefault.p)[k * kEntropyCtxPerSize + i];
    for (unsigned i = 0; i < kLevelsRegionWords; ++i) level[i] = 0;
    EntropyDec d;
    entropy_dec_start(d, bytes, (uint32_t)n_bytes);
    uint32_t count = 0;
    const bool good = entropy_decode_region(d, level, k, ctx, &count);
    if (!good) {
        for (unsigned i = 0; i < kLevelsRegionWords; ++i) level[i] = 0;
        count = 0;
    }
    if (n_nz) *n_nz = count;
    return good ? 0 : 1;
}

// ---- the entropy coder of the motion stream (entropy_kernels.hip, x266_entropy_motion.hpp) and the vectors from the differences (motion_kernels.hip)
int xEntropyEncodeMvGpu(x266hip_ctx *ctx, const x266_entropy_motion_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_motion_encode(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "motion entropy encode launch", launch_entropy_motion_encode(*p, (hipStream_t)stream));
}

int xEntropyDecodeMvGpu(x266hip_ctx *ctx, const x266_entropy_motion_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_motion_decode(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "motion entropy decode launch", launch_entropy_motion_decode(*p, (hipStream_t)stream));
}

int xMotionReconstructGpu(x266hip_ctx *ctx, const x266_motion_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::motion_reconstruct(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "motion reconstruct launch", launch_motion_reconstruct(*p, (hipStream_t)stream));
}

// the three host helpers: the functions of x266_entropy_motion.hpp that the kernels run, on the host
int xEntropyMvDefaultInit(uint16_t init[X266_ENTROPY_MOTION_CONTEXTS])
{
    if (!init) return X266HIP_EINVAL;
    for (unsigned i = 0; i < kEntropyMotionContexts; ++i) init[i] = kEntropyMotionDefault.p[i];
    return X266HIP_OK;
}

int xEntropyEncodeMvCtu(int width, int height, size_t ctu, uint64_t head_mask, const uint16_t *words, const uint16_t *init, uint8_t *out, size_t cap,
                            uint32_t bins[2])
{
    if (args::frame(width, height, 16) || ctu >= args::ctus(width, height) || !words || (!out && cap) || !args::entropy_motion_init_ok(init)) return X266HIP_EINVAL;
    const MotionCtu g = motion_ctu(width / 8, height / 8, ctu);
    if (!motion_mask_well_formed(g, head_mask)) return X266HIP_EINVAL;
    uint16_t c[kEntropyMotionContexts];
    for (unsigned i = 0; i < kEntropyMotionContexts; ++i) c[i] = (init ? init : kEntropyMotionDefault.p)[i];
    EntropyEnc e;
    entropy_enc_start(e, out, cap > kEntropyMotionMaxBytes ? kEntropyMotionMaxBytes : (uint32_t)cap);
    entropy_motion_encode_ctu(e, g, head_mask, words, c);
    const uint32_t n_bytes = entropy_enc_finish(e);
    if (bins) {
        bins[0] = e.ctx_bins;
        bins[1] = e.bypass_bins;
    }
    return (int)n_bytes;
}

int xEntropyDecodeMvCtu(int width, int height, size_t ctu, const uint8_t *bytes, size_t n_bytes, const uint16_t *init, uint64_t *head_mask, uint16_t words[256],
                            uint32_t *parts)
{
    if (args::frame(width, height, 16) || ctu >= args::ctus(width, height) || !head_mask || !words || !parts || (!bytes && n_bytes) ||
        n_bytes > kEntropyMotionMaxBytes || !args::entropy_motion_init_ok(init))
        return X266HIP_EINVAL;
    const MotionCtu g = motion_ctu(width / 8, height / 8, ctu);
    uint16_t c[kEntropyMotionContexts];
    for (unsigned i = 0; i < kEntropyMotionContexts; ++i) c[i] = (init ? init : kEntropyMotionDefault.p)[i];
    for (unsigned i = 0; i < kMotionCtuWords; ++i) words[i] = 0;
    EntropyDec d;
    entropy_dec_start(d, bytes, (uint32_t)n_bytes);
    EntropyMotionCtu r;
    const bool good = entropy_motion_decode_ctu(d, g, c, words, &r);
    if (!good) {
        for (unsigned i = 0; i < kMotionCtuWords; ++i) words[i] = 0;
        entropy_motion_flat_ctu(g, c, words, &r);
    }
    *head_mask = r.mask;
    *parts = r.parts;
    return good ? 0 : 1;
}

// ---- the entropy coder of the side information (entropy_side_kernels.hip, x266_entropy_side.hpp) ------------------------------------------------
int xEntropyEncodeSideGpu(x266hip_ctx *ctx, const x266_entropy_side_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_side_encode(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "side entropy encode launch", launch_entropy_side_encode(*p, (hipStream_t)stream));
}

int xEntropyDecodeSideGpu(x266hip_ctx *ctx, const x266_entropy_side_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_side_decode(p)) return refuse(ctx, __func__, why);
    if (p->n_ctu == 0) return X266HIP_OK;
    X_DEV(ctx);
    return launched(ctx, "side entropy decode launch", launch_entropy_side_decode(*p, (hipStream_t)stream));
}

// the three host helpers: the functions of x266_entropy_side.hpp that the kernels run, on the host
int xEntropySideDefaultInit(uint16_t init[X266_ENTROPY_SIDE_CONTEXTS])
{
    if (!init) return X266HIP_EINVAL;
    for (unsigned i = 0; i < kEntropySideContexts; ++i) init[i] = kEntropySideDefault.p[i];
    return X266HIP_OK;
}

int xEntropyEncodeSideCtu(const uint8_t *kind, const uint8_t *mode, const uint8_t *cls, const uint8_t *qp_in, const uint32_t *nnz, int qp, int chroma_qp_offset,
                          const uint16_t *init, uint8_t *out, size_t cap, uint32_t bins[2])
{
    if ((kind && !mode) || (!out && cap) || !args::entropy_side_scalars_ok(qp, chroma_qp_offset) || !args::entropy_side_init_ok(init)) return X266HIP_EINVAL;
    uint16_t c[kEntropySideContexts];
    for (unsigned i = 0; i < kEntropySideContexts; ++i) c[i] = (init ? init : kEntropySideDefault.p)[i];
    const EntropySideCtu s = entropy_side_canon(kind, mode, cls, qp_in, nnz, qp, chroma_qp_offset);
    EntropyEnc e;
    entropy_enc_start(e, out, cap > kEntropySideMaxBytes ? kEntropySideMaxBytes : (uint32_t)cap);
    entropy_side_encode_ctu(e, s, c, 1u, qp, chroma_qp_offset);
    const uint32_t n_bytes = entropy_enc_finish(e);
    if (bins) {
        bins[0] = e.ctx_bins;
        bins[1] = e.bypass_bins;
    }
    return (int)n_bytes;
}

int xEntropyDecodeSideCtu(const uint8_t *bytes, size_t n_bytes, int qp, int chroma_qp_offset, const uint16_t *init, uint8_t *kind, uint8_t *mode, uint8_t *cls,
                          uint8_t *qp_out, uint32_t *nnz)
{
    if ((!bytes && n_bytes) || n_bytes > kEntropySideMaxBytes || !args::entropy_side_scalars_ok(qp, chroma_qp_offset) || !args::entropy_side_init_ok(init))
        return X266HIP_EINVAL;
    uint16_t c[kEntropySideContexts];
    for (unsigned i = 0; i < kEntropySideContexts; ++i) c[i] = (init ? init : kEntropySideDefault.p)[i];
    EntropyDec d;
    entropy_dec_start(d, bytes, (uint32_t)n_bytes);
    EntropySideCtu s;
    const bool good = entropy_side_decode_ctu(d, c, 1u, qp, chroma_qp_offset, &s);
    if (!good) s = entropy_side_flat_ctu(qp, chroma_qp_offset);
    entropy_side_store(s, kind, mode, cls, qp_out, nnz);
    return good ? 0 : 1;
}

// ---- the per-context bin statistics (entropy_stats_kernels.hip) and the tables from them -----------------------------------------------------------
int xEntropyStatsLevelsGpu(x266hip_ctx *ctx, const x266_entropy_stats_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_stats_levels(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "level statistics launch", launch_entropy_stats_levels(*p, (hipStream_t)stream));
}

int xEntropyStatsSideGpu(x266hip_ctx *ctx, const x266_entropy_side_stats_t *p, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (const char *why = args::entropy_stats_side(p)) return refuse(ctx, __func__, why);
    X_DEV(ctx);
    return launched(ctx, "side statistics launch", launch_entropy_stats_side(*p, (hipStream_t)stream));
}

size_t xEntropyStatsRows(size_t n_units, size_t per_row) { return args::entropy_stats_rows(n_units, per_row); }

int xEntropyInitFromCounts(const uint64_t *counts, size_t n_contexts, uint16_t *init)
{
    if (n_contexts == 0) return X266HIP_OK;
    if (!counts || !init) return X266HIP_EINVAL;
    for (size_t c = 0; c < n_contexts; ++c)
        if ((counts[2 * c] | counts[2 * c + 1]) >> 51) return X266HIP_EINVAL;
    for (size_t c = 0; c < n_contexts; ++c) init[c] = entropy_init_from_counts(counts[2 * c], counts[2 * c + 1]);
    return X266HIP_OK;
}

// the two counting helpers: the walks of x266_entropy.hpp and x266_entropy_side.hpp with the counting sink in place of the coder
int xEntropyCountRegion(const int16_t *level, int cls, int coded, uint64_t counts[2 * X266_ENTROPY_CONTEXTS])
{
    if (!counts || (!level && coded)) return X266HIP_EINVAL;
    const unsigned k = (unsigned)cls & 3u;
    uint16_t ctx[kEntropyCtxPerSize] = {};                                  // the walk's addresses; the sink touches no context
    EntropyCounter<uint64_t, 1> e = {counts + 2u * k * kEntropyCtxPerSize, ctx};
    entropy_encode_region(e, level, k, coded ? entropy_cg_mask(level, k) : 0ull, ctx);
    return X266HIP_OK;
}

int xEntropyCountSideCtu(const uint8_t *kind, const uint8_t *mode, const uint8_t *cls, const uint8_t *qp_in, const uint32_t *nnz, int qp, int chroma_qp_offset,
                         uint64_t counts[2 * X266_ENTROPY_SIDE_CONTEXTS])
{
    if ((kind && !mode) || !counts || !args::entropy_side_scalars_ok(qp, chroma_qp_offset)) return X266HIP_EINVAL;
    uint16_t ctx[kEntropySideContexts] = {};
    EntropyCounter<uint64_t, 1> e = {counts, ctx};
    entropy_side_encode_ctu(e, entropy_side_canon(kind, mode, cls, qp_in, nnz, qp, chroma_qp_offset), ctx, 1u, qp, chroma_qp_offset);
    return X266HIP_OK;
}

// ---- host-pointer batch API --------------------------------------------------
// Chunks of the batch rotate over three staging slots; uploads, kernels and downloads each have a stream of their own
// and are ordered by the slots' events: H2D(i+1) and D2H(i-1) overlap kernel(i).
static int ensure_staging(x266hip_ctx *ctx, size_t in_bytes, size_t out_bytes)
{
    for (hipStream_t &st : ctx->stage_stream)
        if (!st) X_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int i = 0; i < x266hip_ctx::kSlots; ++i) {
        if (!ctx->stage_up[i]) X_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_up[i], hipEventDisableTiming));
        if (!ctx->stage_done[i]) X_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_done[i], hipEventDisableTiming));
        if (!ctx->stage_down[i]) X_HIP(ctx, hipEventCreateWithFlags(&ctx->stage_down[i], hipEventDisableTiming));
    }
    if (in_bytes > ctx->stage_in_bytes) {
        for (int i = 0; i < x266hip_ctx::kSlots; ++i) {
            if (ctx->d_stage_in[i]) (void)hipFree(ctx->d_stage_in[i]);
            ctx->d_stage_in[i] = nullptr;
            if (hipMalloc(&ctx->d_stage_in[i], in_bytes) != hipSuccess) { ctx->stage_in_bytes = 0; return fail(ctx, X266HIP_ENOMEM, "staging alloc"); }
        }
        ctx->stage_in_bytes = in_bytes;
    }
    if (out_bytes > ctx->stage_out_bytes) {
        for (int i = 0; i < x266hip_ctx::kSlots; ++i) {
            if (ctx->d_stage_out[i]) (void)hipFree(ctx->d_stage_out[i]);
            ctx->d_stage_out[i] = nullptr;
            if (hipMalloc(&ctx->d_stage_out[i], out_bytes) != hipSuccess) { ctx->stage_out_bytes = 0; return fail(ctx, X266HIP_ENOMEM, "staging alloc"); }
        }
        ctx->stage_out_bytes = out_bytes;
    }
    return X266HIP_OK;
}

// Uploads + kernels are issued by the calling thread, downloads by a helper thread that lives for the call: a copy from / to
// PAGEABLE memory blocks the thread that issues it while the runtime stages it, so one thread keeps only one direction of the
// link busy (27 GB/s each way); two threads reach what pinned buffers reach, 43-44 GB/s each way of the 48.5 the link gives
// with both directions running (profiles/r04_hostpipe.txt).
static int host_batch(x266hip_ctx *ctx, int op, const void *in, void *out, size_t n, size_t in_unit, size_t out_unit)
{
    if (!ctx) return X266HIP_EINVAL;
    if (n == 0) return X266HIP_OK;
    if (!in || !out) return fail(ctx, X266HIP_EINVAL, "NULL host buffer");
    X_DEV(ctx);
    // A call of a block or a few (the BDPI shims hand over ONE: dct32_genNew, satd8x8_genNew) is all latency: upload, kernel and download
    // as three stream operations cost 60-80 us per call.  Up to 64 KiB each way the kernel instead reads its input from, and writes its result
    // to, page-locked host memory the device sees (hipHostMalloc: coherent, uncached on the device side): two memcpy on the host, ONE launch,
    // one synchronize -- profiles/r06_bdpi_latency.txt.  Same kernels, same bytes (tests/test_gpu_parity.py runs both paths against each other).
    if (n * in_unit <= x266hip_ctx::kSmallCallBytes && n * out_unit <= x266hip_ctx::kSmallCallBytes) {
        if (!ctx->h_small_in) X_HIP(ctx, hipHostMalloc(&ctx->h_small_in, x266hip_ctx::kSmallCallBytes, hipHostMallocDefault));
        if (!ctx->h_small_out) X_HIP(ctx, hipHostMalloc(&ctx->h_small_out, x266hip_ctx::kSmallCallBytes, hipHostMallocDefault));
        if (!ctx->small_stream) X_HIP(ctx, hipStreamCreateWithFlags(&ctx->small_stream, hipStreamNonBlocking));
        std::memcpy(ctx->h_small_in, in, n * in_unit);
        const int rc_small = launch_op(ctx, op, ctx->h_small_in, ctx->h_small_out, n, ctx->small_stream);
        const hipError_t es = hipStreamSynchronize(ctx->small_stream);   // also after a failed launch: nothing of this call stays in flight
        if (rc_small != X266HIP_OK) return rc_small;
        if (es != hipSuccess) return fail(ctx, X266HIP_EDEVICE, "hipStreamSynchronize(small call)", es);
        std::memcpy(out, ctx->h_small_out, n * out_unit);
        return X266HIP_OK;
    }
    const size_t chunk_bytes = (size_t)16 << 20;                       // 16 MiB of input per chunk
    size_t chunk = chunk_bytes / in_unit;
    if (chunk > n) chunk = n;
    int rc = ensure_staging(ctx, chunk * in_unit, chunk * out_unit);
    if (rc) return rc;
    hipStream_t s_up = ctx->stage_stream[0], s_k = ctx->stage_stream[1], s_down = ctx->stage_stream[2];
    const size_t n_chunks = (n + chunk - 1) / chunk;
    constexpr long kSlots = x266hip_ctx::kSlots;

    struct Shared {
        std::mutex m;
        std::condition_variable cv;
        long launched = 0, drained = 0;                               // chunks whose kernel is enqueued / whose results have arrived
        bool stop = false;                                            // a failure on either side: both loops leave
        hipError_t down_error = hipSuccess;
    } sh;

    std::thread down;
    if (n_chunks > 1) try {
        down = std::thread([&]() {
            (void)hipSetDevice(ctx->device);
            for (size_t i = 0; i < n_chunks; ++i) {
                {
                    std::unique_lock<std::mutex> lk(sh.m);
                    sh.cv.wait(lk, [&] { return sh.stop || sh.launched > (long)i; });
                    if (sh.launched <= (long)i) return;              // stopped before this chunk was issued
                }
                const int slot = (int)(i % kSlots);
                const size_t done = i * chunk, cnt = n - done < chunk ? n - done : chunk;
                hipError_t e = hipStreamWaitEvent(s_down, ctx->stage_done[slot], 0);
                if (e == hipSuccess) e = hipMemcpyAsync((char *)out + done * out_unit, ctx->d_stage_out[slot], cnt * out_unit, hipMemcpyDeviceToHost, s_down);
                if (e == hipSuccess) e = hipStreamSynchronize(s_down);
                std::lock_guard<std::mutex> lk(sh.m);
                if (e != hipSuccess) { sh.down_error = e; sh.stop = true; }
                sh.drained = (long)i + 1;
                sh.cv.notify_all();
                if (e != hipSuccess) return;
            }
        });
    } catch (const std::system_error &) {                               // no thread to be had: nothing has been issued yet
        return fail(ctx, X266HIP_ENOMEM, "could not start the download thread of a host-pointer batch call");
    }
    hipError_t e = hipSuccess;
    const char *what = "";
#define STAGE(call) do { if (e == hipSuccess && rc == X266HIP_OK) { e = (call); what = #call; } } while (0)
    for (size_t i = 0; i < n_chunks && e == hipSuccess && rc == X266HIP_OK; ++i) {
        const int slot = (int)(i % kSlots);
        const size_t done = i * chunk, cnt = n - done < chunk ? n - done : chunk;
        if (n_chunks > 1) {                                             // the slot's previous chunk has left
            std::unique_lock<std::mutex> lk(sh.m);
            sh.cv.wait(lk, [&] { return sh.stop || (long)i - sh.drained < kSlots; });
            if (sh.stop) break;
        }
        STAGE(hipMemcpyAsync(ctx->d_stage_in[slot], (const char *)in + done * in_unit, cnt * in_unit, hipMemcpyHostToDevice, s_up));
        STAGE(hipEventRecord(ctx->stage_up[slot], s_up));
        STAGE(hipStreamWaitEvent(s_k, ctx->stage_up[slot], 0));
        if (e == hipSuccess) rc = launch_op(ctx, op, ctx->d_stage_in[slot], ctx->d_stage_out[slot], cnt, s_k);
        STAGE(hipEventRecord(ctx->stage_done[slot], s_k));
        if (n_chunks == 1) {                                            // a small call: no helper thread, the download follows in stream order
            STAGE(hipStreamWaitEvent(s_down, ctx->stage_done[slot], 0));
            STAGE(hipMemcpyAsync(out, ctx->d_stage_out[slot], cnt * out_unit, hipMemcpyDeviceToHost, s_down));
        } else if (e == hipSuccess && rc == X266HIP_OK) {
            std::lock_guard<std::mutex> lk(sh.m);
            sh.launched = (long)i + 1;
            sh.cv.notify_all();
        }
    }
#undef STAGE
    if (down.joinable()) {
        {
            std::lock_guard<std::mutex> lk(sh.m);
            if (e != hipSuccess || rc != X266HIP_OK) sh.stop = true;
            sh.cv.notify_all();
        }
        down.join();                                                    // it leaves once every issued chunk has been downloaded (or on a failure)
    }
    // Drain EVERY staging stream on every path: after a failure an already enqueued D2H copy must not still be
    // writing the caller's `out` once this function has returned (the caller may free it).
    for (hipStream_t st : ctx->stage_stream) {
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess && es != hipSuccess) { e = es; what = "hipStreamSynchronize(stage)"; }
    }
    if (rc != X266HIP_OK) return rc;
    if (e == hipSuccess && sh.down_error != hipSuccess) { e = sh.down_error; what = "download (helper thread)"; }
    if (e != hipSuccess) return fail(ctx, X266HIP_EDEVICE, what, e);
    return X266HIP_OK;
}

int xDct32FwdBatch(x266hip_ctx *ctx, const int16_t *in, int16_t *out, size_t n) { return host_batch(ctx, 0, in, out, n, 2048, 2048); }
int xDct32InvBatch(x266hip_ctx *ctx, const int16_t *in, int16_t *out, size_t n) { return host_batch(ctx, 1, in, out, n, 2048, 2048); }
int xSatd8x8Batch(x266hip_ctx *ctx, const int16_t *diff, uint32_t *out, size_t n) { return host_batch(ctx, 2, diff, out, n, 128, 4); }

// ---- memory / stream helpers ---------------------------------------------------
int xHipMalloc(x266hip_ctx *ctx, void **d_ptr, size_t bytes)
{
    if (!ctx || !d_ptr) return X266HIP_EINVAL;
    X_DEV(ctx);
    *d_ptr = nullptr;
    if (bytes == 0) return X266HIP_OK;
    hipError_t e = hipMalloc(d_ptr, bytes);
    if (e != hipSuccess) return fail(ctx, X266HIP_ENOMEM, "hipMalloc", e);
    return X266HIP_OK;
}

int xHipHostAlloc(x266hip_ctx *ctx, void **h_ptr, size_t bytes)
{
    if (!ctx || !h_ptr) return X266HIP_EINVAL;
    X_DEV(ctx);
    *h_ptr = nullptr;
    if (bytes == 0) return X266HIP_OK;
    hipError_t e = hipHostMalloc(h_ptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, X266HIP_ENOMEM, "hipHostMalloc", e);
    return X266HIP_OK;
}

int xHipHostFree(x266hip_ctx *ctx, void *h_ptr)
{
    if (!ctx) return X266HIP_EINVAL;
    if (!h_ptr) return X266HIP_OK;
    X_DEV(ctx);
    X_HIP(ctx, hipHostFree(h_ptr));
    return X266HIP_OK;
}

int xHipFree(x266hip_ctx *ctx, void *d_ptr)
{
    if (!ctx) return X266HIP_EINVAL;
    if (!d_ptr) return X266HIP_OK;
    X_DEV(ctx);
    X_HIP(ctx, hipFree(d_ptr));
    return X266HIP_OK;
}

int xHipMemcpyH2D(x266hip_ctx *ctx, void *d_dst, const void *src, size_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !src))) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return X266HIP_OK;
}

int xHipMemcpyD2H(x266hip_ctx *ctx, void *dst, const void *d_src, size_t bytes)
{
    if (!ctx || (bytes && (!dst || !d_src))) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return X266HIP_OK;
}

int xHipStreamSync(x266hip_ctx *ctx, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return X266HIP_OK;
}

int xHipStreamCreate(x266hip_ctx *ctx, void **stream)
{
    if (!ctx || !stream) return X266HIP_EINVAL;
    X_DEV(ctx);
    hipStream_t s = nullptr;
    X_HIP(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return X266HIP_OK;
}

int xHipStreamDestroy(x266hip_ctx *ctx, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (!stream) return X266HIP_OK;
    X_DEV(ctx);
    X_HIP(ctx, hipStreamDestroy((hipStream_t)stream));
    return X266HIP_OK;
}

struct x266hip_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

int xHipGraphBegin(x266hip_ctx *ctx, void *stream)
{
    if (!ctx) return X266HIP_EINVAL;
    if (!stream) return fail(ctx, X266HIP_EINVAL, "xHipGraphBegin: capture needs a stream of its own, not the NULL stream");
    X_DEV(ctx);
    X_HIP(ctx, hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    return X266HIP_OK;
}

int xHipGraphEnd(x266hip_ctx *ctx, void *stream, x266hip_graph **graph)
{
    if (!ctx || !graph || !stream) return X266HIP_EINVAL;
    *graph = nullptr;
    X_DEV(ctx);
    hipGraph_t g = nullptr;
    X_HIP(ctx, hipStreamEndCapture((hipStream_t)stream, &g));
    if (!g) return fail(ctx, X266HIP_EDEVICE, "xHipGraphEnd: the capture was invalidated");
    hipGraphExec_t e = nullptr;
    const hipError_t rc = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    if (rc != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fail(ctx, X266HIP_EDEVICE, "hipGraphInstantiate", rc);
    }
    x266hip_graph *out = new (std::nothrow) x266hip_graph;
    if (!out) {
        (void)hipGraphExecDestroy(e);
        (void)hipGraphDestroy(g);
        return X266HIP_ENOMEM;
    }
    out->graph = g;
    out->exec = e;
    *graph = out;
    return X266HIP_OK;
}

int xHipGraphLaunch(x266hip_ctx *ctx, x266hip_graph *graph, void *stream)
{
    if (!ctx || !graph || !graph->exec) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipGraphLaunch(graph->exec, (hipStream_t)stream));
    return X266HIP_OK;
}

void xHipGraphFree(x266hip_ctx *ctx, x266hip_graph *graph)
{
    if (!graph) return;
    DeviceScope dev_scope_(ctx ? ctx->device : 0);
    if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
    if (graph->graph) (void)hipGraphDestroy(graph->graph);
    delete graph;
}

int xHipEventCreate(x266hip_ctx *ctx, void **event)
{
    if (!ctx || !event) return X266HIP_EINVAL;
    X_DEV(ctx);
    hipEvent_t e = nullptr;
    X_HIP(ctx, hipEventCreate(&e));
    *event = (void *)e;
    return X266HIP_OK;
}

int xHipEventDestroy(x266hip_ctx *ctx, void *event)
{
    if (!ctx) return X266HIP_EINVAL;
    if (!event) return X266HIP_OK;
    X_DEV(ctx);
    X_HIP(ctx, hipEventDestroy((hipEvent_t)event));
    return X266HIP_OK;
}

int xHipEventRecord(x266hip_ctx *ctx, void *event, void *stream)
{
    if (!ctx || !event) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return X266HIP_OK;
}

int xHipEventElapsedMs(x266hip_ctx *ctx, void *start, void *stop, double *ms)
{
    if (!ctx || !start || !stop || !ms) return X266HIP_EINVAL;
    X_DEV(ctx);
    X_HIP(ctx, hipEventSynchronize((hipEvent_t)stop));
    float f = 0.f;
    X_HIP(ctx, hipEventElapsedTime(&f, (hipEvent_t)start, (hipEvent_t)stop));
    *ms = (double)f;
    return X266HIP_OK;
}

int xHipTimeKernel(x266hip_ctx *ctx, int op, const void *d_in, void *d_out, size_t n, int reps, void *stream,
                   double *ms_per_launch)
{
    if (!ctx || !ms_per_launch || reps < 1) return X266HIP_EINVAL;
    X_DEV(ctx);
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    X_HIP(ctx, hipEventCreate(&e0));
    X_HIP(ctx, hipEventCreate(&e1));
    int rc = X266HIP_OK;
    hipError_t e = hipEventRecord(e0, s);
    for (int i = 0; i < reps && rc == X266HIP_OK && e == hipSuccess; ++i) rc = launch_op(ctx, op, d_in, d_out, n, s);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, X266HIP_EDEVICE, "event timing", e);
    *ms_per_launch = (double)ms / reps;
    return X266HIP_OK;
}

}  // extern "C"
