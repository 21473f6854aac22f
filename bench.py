#!/usr/bin/env python3
"""bench.py -- throughput of the x266 DCT32 / SATD hot path on MI355X.

Contract (one JSON line on stdout from rank 0):
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  N > 1 is launched by the driver as
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
  (plain `python bench.py --gpus N` without WORLD_SIZE in the environment spawns exactly that itself)

Workload = BASELINE.json configs[1]: 1,048,576 synthetic 9-bit residual blocks of 32x32 int16 per GPU, resident in HBM
before the timed region (values a-b, a,b uniform bytes -- the reference's stimulus distribution, src_tb/dct32.c:191-193 --
from SplitMix64 seed 0x266).  A "step" is one forward 2-D DCT32 pass over the batch (xDct32FwdBatchDev through the C ABI).
`value` is whole-job forward blocks/s over all ranks.

A plain run does only what that figure needs: set-up, warm-up, the K timed steps, the outputs (--dump-outputs) and the line.
Everything else is behind --full: the same-box memory streams, the live counter passes behind roofline.traffic, the output
checksum over ranks, the CPU baseline, and every other leg (inverse, fused forward+inverse, the 8x8 SATD residual batch of
2^24 blocks, motion search, the transform set, the 8K frame stream of configs[4], ...), each one function below, measured
the same way, under "also".

--dump-outputs DIR: after the timed steps, rank 0 writes what the last step computed as DIR/dct32_fwd_coefficients.npy,
float32 [S, 1024] -- the coefficients of S = min(8192, blocks per GPU) blocks of its shard, chosen by a fixed seed and kept in
block order (32 MiB at most).  The inputs come from a fixed seed too, so two builds run with the same arguments can be
compared output for output.

The process runs on the runtime the library ships on: device memory, streams and events come from the C ABI (xHipMalloc,
xHipMemcpy*, xHipEvent*) and, for the two raw link copies of the host-API leg, from the HIP runtime libx266hip.so itself
loaded (ctypes) -- no torch in the single-GPU path.  With N > 1, torch.distributed is the CONTROL plane only, on gloo,
imported after the library: barrier, max-over-ranks time, checksum sum, the broadcast of the node's RCCL id; the data path
(RCCL send/recv groups of the node layer, x266_amd/csrc/x266hip_node.cpp) then talks to ROCm's librccl, not the older copy
the torch wheel bundles.  `hip_runtime` / `rccl_by_rank` in the line say which libraries the process really had.

How every leg is timed (`Bench.timed_leg`): its own clock pre-warm (the chip needs ~50 ms of load to reach steady clocks,
profiles/r01_clock_warmup.txt), W untimed launches, then K launches between barrier + device synchronize on both sides; a HIP
event is recorded ON THE LAUNCHING STREAM before every one of those K launches and after the last, so the kernel durations
come from the very launches whose wall-clock is `ms_per_step`.  Fractions use `kernel_ms` = the 10 % trimmed mean of those K
durations (a profiler's or the host's hiccup on 1 launch in 20 must not move a fraction by 2x: round 4's sad_8x8 row);
the plain mean and the median are reported next to it.

"roofline": algorithmic bytes per launch (4096 B per DCT block, 132 B per SATD block) / kernel_ms,
against the 8 TB/s HBM3E peak.  "cpu_baseline": the reference C path on this node's host cores (oracle/_ref = the real
src_tb/dct32.c when its prebuilt .so is present, else the oracle's restatement), rank 0 at N = 1 only.  The oracle is used
there and nowhere in the product.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_cpu import cpu_baseline_dct                                                        # noqa: E402  (the cpu_baseline leg)
from bench_legs import (HBM_PEAK_BYTES_PER_S, DCT_BYTES_PER_BLOCK, DCT_SEED,                # noqa: E402,F401
                        leg_dct32_inverse_and_fused, leg_autotuned, leg_satd, leg_motion_search, leg_transform_set, leg_fused_from_tiles,
                        leg_front_end_and_sad, leg_intra, leg_host_api, run_node_legs_under_watchdog)

DCT_BLOCKS_PER_GPU = 1 << 20           # BASELINE configs[1]
SATD_BLOCKS_PER_GPU = 1 << 24          # 2 GiB of 8x8 residual blocks
PREWARM_SECONDS = 0.08
P = ctypes.c_void_p


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dct-blocks", type=int, default=DCT_BLOCKS_PER_GPU)
    ap.add_argument("--satd-blocks", type=int, default=SATD_BLOCKS_PER_GPU)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-also", action="store_true", help="headline leg only")
    ap.add_argument("--stream8k", type=int, default=200, metavar="FRAMES",
                    help="frames of the BASELINE configs[4] leg (7680x4320 stream through the node layer); 0 skips it")
    ap.add_argument("--node-timeout", type=float, default=240.0,
                    help="seconds the node-layer legs (RCCL) may take before the JSON line is printed without them")
    ap.add_argument("--no-me", action="store_true", help="skip the motion-search legs")
    ap.add_argument("--no-host-api", action="store_true", help="skip the PCIe-inclusive host-pointer leg")
    ap.add_argument("--no-transform-set", action="store_true", help="skip the transform-set / front-end / intra legs")
    ap.add_argument("--no-autotune", action="store_true", help="skip the default-vs-autotuned leg (profiled runs: its candidate launches would mix shapes into the per-kernel averages)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not run the two rocprofv3 --pmc passes that measure roofline.traffic (replay profiles/traffic.json instead)")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)   # the profiled child of the live traffic passes
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline (same-box streams, live traffic passes, checksum, CPU baseline, 'also'); "
                         "the --no-* options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write a fixed, seeded sample of the last timed step's output to DIR/dct32_fwd_coefficients.npy (float32)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------
# the HIP runtime of this process (the copy libx266hip.so loaded), through ctypes
# ------------------------------------------------------------------------------------------------
def loaded_libraries(prefix):
    """paths of the shared objects mapped into this process whose file name starts with `prefix`"""
    seen = []
    for line in open("/proc/self/maps"):
        parts = line.split()
        if len(parts) >= 6 and parts[5].rsplit("/", 1)[-1].startswith(prefix) and parts[5] not in seen:
            seen.append(parts[5])
    return seen


class HipRuntime:
    """what bench.py needs of HIP beyond the C ABI: device synchronize, the PCI address, raw async copies for the link's own rate"""

    def __init__(self):
        self.paths = loaded_libraries("libamdhip64.so")
        if not self.paths:
            raise SystemExit("libx266hip.so did not bring a HIP runtime into the process")
        self.lib = L = ctypes.CDLL(self.paths[0])
        L.hipMemcpyAsync.argtypes = [P, P, ctypes.c_size_t, ctypes.c_int, P]
        L.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(P), ctypes.c_uint]
        L.hipStreamSynchronize.argtypes = [P]
        L.hipStreamDestroy.argtypes = [P]
        L.hipDeviceGetPCIBusId.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def device_sync(self):
        self.check(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def version(self):
        v = ctypes.c_int()
        self.check(self.lib.hipRuntimeGetVersion(ctypes.byref(v)), "hipRuntimeGetVersion")
        return v.value

    def pci_bus_id(self, device):
        buf = ctypes.create_string_buffer(64)
        return buf.value.decode().lower() if self.lib.hipDeviceGetPCIBusId(buf, 64, device) == 0 else None

    def stream_create(self):
        s = P()
        self.check(self.lib.hipStreamCreateWithFlags(ctypes.byref(s), 1), "hipStreamCreateWithFlags")   # hipStreamNonBlocking
        return s

    def memcpy_async(self, dst, src, nbytes, kind, stream):
        self.check(self.lib.hipMemcpyAsync(P(dst), P(src), nbytes, kind, stream), "hipMemcpyAsync")


# ------------------------------------------------------------------------------------------------
# roofline.traffic, live: HBM bytes of one headline launch from the PMC counters, collected as
# MI355X_MICROARCH.md prescribes -- FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 passes with --kernel-trace only
# (never with sys / hip / hsa traces), units KB.  gfx950's FETCH_SIZE counts the 128-byte requests of 16 B-per-lane
# streaming reads as 64 B; the factor is not assumed but CALIBRATED IN THE SAME PASS on a kernel whose read volume is
# known by construction (xHipMemCeilingDev's copy of the same buffer: it reads exactly n * 2048 bytes), so the headline
# kernel's figure does not rest on its own algorithmic byte count.
# ------------------------------------------------------------------------------------------------
def traffic_child(args):
    """what the profiled passes run: the calibration copy and the headline launch on the full batch, a few times, nothing else"""
    import x266_amd
    codec = x266_amd.Codec(0)
    n = args.dct_blocks
    x, z = codec.alloc(n * 2048), codec.alloc(n * 2048)
    codec.fill_residual_dev(x.ptr, n * 1024, DCT_SEED, 0, 0)
    for _ in range(3):
        codec.mem_ceiling_dev(0, x.ptr, z.ptr, n * 2048, 0)
    for _ in range(6):
        codec.dct32_fwd_dev(x.ptr, z.ptr, n, 0)
    codec.stream_sync()


def measure_traffic_live(n_dct, budget_s=150.0):
    """(bytes per headline launch, how it was measured) or (None, why not)"""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    # already running under a profiler (someone profiles this bench run): do not nest a second one
    if any(k.startswith(("ROCPROF", "ROCP_", "ROCTRACER")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None, "this process is itself being profiled (ROCPROF* / ROCP_* in the environment)"
    t0 = time.time()
    kb, cal = {}, {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="x266_pmc_", dir="/tmp")
        try:
            env = dict(os.environ, TMPDIR="/tmp")
            left = budget_s - (time.time() - t0)
            if left < 20:
                return None, "time budget of the live traffic passes exhausted"
            subprocess.run([exe, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--traffic-child", "--dct-blocks", str(n_dct)],
                           cwd="/tmp", env=env, timeout=left, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            vals, cvals = [], []
            for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    name = r.get("Kernel_Name", "").replace(" ", "")
                    if r.get("Counter_Name") != ctr:
                        continue
                    if "dct32_lds_kernel<false>" in name or "dct32_lds_kernel<0" in name:
                        vals.append(float(r["Counter_Value"]))
                    elif "mem_ceiling_kernel<0" in name:
                        cvals.append(float(r["Counter_Value"]))
            if not vals:
                return None, "no %s rows for the forward kernel in rocprofv3's output" % ctr
            kb[ctr] = sum(vals) / len(vals)
            cal[ctr] = (sum(cvals) / len(cvals)) if cvals else None
        except Exception as e:                                            # a profiler that cannot run must not cost the bench line
            return None, "rocprofv3 --pmc %s failed: %s" % (ctr, str(e)[:120])
        finally:
            shutil.rmtree(d, ignore_errors=True)
    known = n_dct * 2048.0                                                # what the calibration copy reads and writes, by construction
    f_fetch = known / (cal["FETCH_SIZE"] * 1024.0) if cal["FETCH_SIZE"] else 2.0
    f_write = known / (cal["WRITE_SIZE"] * 1024.0) if cal["WRITE_SIZE"] else 1.0
    total = kb["FETCH_SIZE"] * 1024.0 * f_fetch + kb["WRITE_SIZE"] * 1024.0 * f_write
    return total, ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes) around 6 launches of the headline kernel on "
                   "this batch; KB x 1024 x a factor calibrated in the same pass on xHipMemCeilingDev's copy of the same buffer (known to read and write %d bytes): "
                   "FETCH_SIZE x %.4f%s, WRITE_SIZE x %.4f%s; raw: headline FETCH_SIZE %.1f KB, WRITE_SIZE %.1f KB per launch; %.0f s"
                   % (int(known), f_fetch, "" if cal["FETCH_SIZE"] else " (calibration rows missing: the guide's gfx950 factor)", f_write,
                      "" if cal["WRITE_SIZE"] else " (calibration rows missing)", kb["FETCH_SIZE"], kb["WRITE_SIZE"], time.time() - t0))


# ------------------------------------------------------------------------------------------------
# sysfs facts of the device (matched by PCI address: a box shows every GPU of the host, not only its own)
# ------------------------------------------------------------------------------------------------
def gpu_sysfs_dir(pci):
    import glob
    if not pci:
        return None
    for dev in sorted(glob.glob("/sys/class/drm/card*/device")):
        if os.path.realpath(dev).split("/")[-1].lower() == pci:
            return dev
    return None


def trimmed_mean(d, frac=0.10):
    """mean of the middle 1 - 2 frac of the sorted durations"""
    s = sorted(d)
    k = int(len(s) * frac)
    s = s[k:len(s) - k] if len(s) - 2 * k >= 1 else s
    return sum(s) / len(s)


# ------------------------------------------------------------------------------------------------
# the run: device, ranks, timing helpers
# ------------------------------------------------------------------------------------------------
def pick_device(local_rank, n_dev, share, env):
    """HIP device ordinal of the rank torchrun calls LOCAL_RANK: one process per GPU, rank i on device i.  A launcher that instead narrows
    every rank to ONE visible device (HIP_/ROCR_/CUDA_VISIBLE_DEVICES set per process) leaves ordinal 0 as the rank's own.  Anything
    else with fewer devices than ranks is a launch error, said here rather than as a failed hipSetDevice."""
    if share:
        return local_rank % n_dev
    if local_rank < n_dev:
        return local_rank
    if n_dev == 1 and any(env.get(k) for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")):
        return 0
    raise SystemExit("LOCAL_RANK %d but only %d HIP device(s) visible: bench.py runs one rank per GPU" % (local_rank, n_dev))


class Bench:
    def __init__(self, args):
        import x266_amd                                                 # the library first: ITS HIP runtime is the process's
        self.args = args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:
            raise SystemExit("--gpus %d but WORLD_SIZE is %d: launch one rank per GPU (or run without torch.distributed.run: bench.py spawns its own ranks)" % (args.gpus, self.world))
        n_dev = int(x266_amd.load_library().xHipDeviceCount())
        if n_dev < 1:
            raise SystemExit("bench.py needs an MI355X: libx266hip has no CPU path")
        # Test hook (never set by the driver): X266_BENCH_SHARE_GPU=1 lets several ranks share the visible GPUs, so that the N > 1 code
        # path -- shard offsets, max-over-ranks timing, checksum reduction -- can be exercised on a one-GPU box.  RCCL refuses two ranks
        # on one device, so the node-layer legs run there only when X266HIP_RCCL_LIB names the tests' RCCL model.
        self.share = os.environ.get("X266_BENCH_SHARE_GPU") == "1"
        self.local_rank = pick_device(local_rank, n_dev, self.share, os.environ)
        self.codec = x266_amd.Codec(self.local_rank)
        self.hip = HipRuntime()
        self.hip.check(self.hip.lib.hipSetDevice(self.local_rank), "hipSetDevice")
        self.dist = None
        if self.world > 1:                                              # control plane only, on gloo, AFTER the library (module docstring)
            import torch.distributed as dist
            import torch
            self.torch = torch
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
            self.dist = dist
        self.K, self.W = args.steps, args.warmup
        self.n_dct, self.n_satd = args.dct_blocks, args.satd_blocks
        self.stream = 0                                                 # every launch and event of the legs: the NULL stream
        self.events = [self.codec.event_create() for _ in range(max(self.K, 64) + 1)]
        self.info = self.codec.device_info()
        self.sysfs = gpu_sysfs_dir(self.hip.pci_bus_id(self.local_rank))
        self.ceil = {}                                                  # this box's streams, bytes per second (leg_same_box)
        self._keep = []

    # -- device memory through the C ABI -----------------------------------------------------------
    def dev(self, nbytes):
        return self.codec.alloc(max(int(nbytes), 16))

    def dev_from(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.dev(arr.nbytes)
        b.upload(arr)
        return b

    def dev_random_bytes(self, nbytes, seed):
        """uniform low bytes, sign-extension high bytes (the residual stream seen as bytes): contents never steer a kernel here"""
        b = self.dev(nbytes)
        self.codec.fill_residual_dev(b.ptr, nbytes // 2, seed, 0, self.stream)
        return b

    # -- control plane ------------------------------------------------------------------------------
    def barrier(self):
        self.hip.device_sync()
        if self.dist is not None:
            self.dist.barrier()
            self.hip.device_sync()

    def max_over_ranks(self, seconds):
        if self.dist is None:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_ranks(self, value):
        """the value of every rank, in rank order (control-plane all-gather)"""
        if self.dist is None:
            return [value]
        t = self.torch.zeros(self.world, dtype=self.torch.float64)
        t[self.rank] = value
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    def sum_over_ranks_i64(self, value):
        if self.dist is None:
            return int(value)
        t = self.torch.tensor([int(value)], dtype=self.torch.int64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return int(t.item())

    # -- timing ---------------------------------------------------------------------------------------
    def timed_leg(self, fn, steps=None, warmup=None):
        """fn() enqueues one step on the NULL stream.  Returns dict(wall_s, ms_per_step, kernel_ms (trimmed mean), kernel_ms_mean, kernel_ms_median)."""
        codec, events = self.codec, self.events
        steps = self.K if steps is None else max(1, min(steps, len(events) - 1))
        warmup = self.W if warmup is None else warmup
        self.hip.device_sync()                                          # clock pre-warm: a few launches to size one step, then ~PREWARM_SECONDS of load
        t0 = time.perf_counter()
        for _ in range(2):
            fn()
        self.hip.device_sync()
        per = max((time.perf_counter() - t0) / 2, 1e-6)
        pre = min(2000, int(PREWARM_SECONDS / per))
        for _ in range(pre + warmup):
            fn()
        self.barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            codec.event_record(events[i], self.stream)
            fn()
        codec.event_record(events[steps], self.stream)
        self.barrier()
        wall = self.max_over_ranks(time.perf_counter() - t0)
        d = [codec.event_elapsed_ms(events[i], events[i + 1]) for i in range(steps)]
        # kernel time like wall time: the slowest rank's (every rank runs the same launches on its own shard)
        trim_all = self.all_ranks(trimmed_mean(d))
        return {"wall_s": wall, "steps": steps, "ms_per_step": wall / steps * 1e3, "kernel_ms": max(trim_all),
                "kernel_ms_mean": max(self.all_ranks(sum(d) / steps)), "kernel_ms_median": max(self.all_ranks(statistics.median(d))),
                "kernel_ms_by_rank": trim_all if self.world > 1 else None, "clock_prewarm_launches": pre}

    def rate(self, leg, units_per_step):
        return self.world * units_per_step * leg["steps"] / leg["wall_s"]

    def of_box(self, achieved_bytes_per_s, kind):
        """fraction of this box's own stream of that kind (None in a plain run: the same-box streams are measured under --full)"""
        return achieved_bytes_per_s / self.ceil[kind] if kind in self.ceil else None

    def hbm(self, leg, bytes_per_step, box_kind="copy"):
        """{hbm_frac, frac_of_same_box_<kind>} of a leg, from the trimmed mean of its launches"""
        achieved = bytes_per_step / (leg["kernel_ms"] * 1e-3)
        return {"hbm_frac": achieved / HBM_PEAK_BYTES_PER_S, "frac_of_same_box_%s" % box_kind: self.of_box(achieved, box_kind)}

    def roofline(self, leg, bytes_per_unit, n_units, traffic=None, traffic_source=None, box_kind="copy"):
        per_launch = bytes_per_unit * n_units
        achieved = per_launch / (leg["kernel_ms"] * 1e-3)
        return {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK_BYTES_PER_S / 1e9, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_BYTES_PER_S, "frac_of_same_box_%s" % box_kind: self.of_box(achieved, box_kind),
                "traffic": traffic, "traffic_source": traffic_source,
                "kernel_ms_per_launch": leg["kernel_ms"], "kernel_ms_mean": leg["kernel_ms_mean"], "kernel_ms_median": leg["kernel_ms_median"],
                "kernel_ms_per_launch_is": "10 % trimmed mean of the HIP-event durations of the timed launches (events on the launching stream); with several ranks the slowest rank's",
                "frac_by_rank": [per_launch / (m * 1e-3) / HBM_PEAK_BYTES_PER_S for m in leg["kernel_ms_by_rank"]] if leg.get("kernel_ms_by_rank") else None,
                "frac_at_mean": per_launch / (leg["kernel_ms_mean"] * 1e-3) / HBM_PEAK_BYTES_PER_S,
                "frac_at_median": per_launch / (leg["kernel_ms_median"] * 1e-3) / HBM_PEAK_BYTES_PER_S,
                "algorithmic_bytes_per_launch": per_launch}

    @staticmethod
    def brief(leg):
        return {k: leg[k] for k in ("ms_per_step", "kernel_ms", "kernel_ms_mean", "kernel_ms_median")}

    def same_on_device(self, a, b, nbytes, chunk=256 << 20):
        """two device buffers hold the same bytes (downloaded in chunks and compared on the host)"""
        for off in range(0, nbytes, chunk):
            n = min(chunk, nbytes - off)
            ha, hb = np.empty(n, np.uint8), np.empty(n, np.uint8)
            self.codec._check(self.codec.L.xHipMemcpyD2H(self.codec.ctx, ha.ctypes.data, a.ptr + off, n), "xHipMemcpyD2H")
            self.codec._check(self.codec.L.xHipMemcpyD2H(self.codec.ctx, hb.ctypes.data, b.ptr + off, n), "xHipMemcpyD2H")
            if not np.array_equal(ha, hb):
                return False
        return True


# ------------------------------------------------------------------------------------------------
# the legs: the headline's own below; every other family is one function of tools/bench_legs.py
# ------------------------------------------------------------------------------------------------
def leg_same_box(b, x, z):
    """What THIS box's memory system gives the streaming launch shapes, with no arithmetic (xHipMemCeilingDev): the same-run reference
    every HBM-bound leg is also expressed in, because boxes of the pool differ by 3-10 % in what a plain stream reaches."""
    ceil_bytes = b.n_dct * 2048
    for kind, name, moved in ((0, "copy", 2 * ceil_bytes), (1, "read", ceil_bytes), (3, "read_probe", ceil_bytes), (2, "write", ceil_bytes)):
        leg = b.timed_leg(lambda k=kind: b.codec.mem_ceiling_dev(k, x.ptr, z.ptr, ceil_bytes, b.stream), steps=min(b.K, 40), warmup=min(b.W, 10))
        b.ceil[name] = moved / (leg["kernel_ms"] * 1e-3)
    return {"copy_TBps": b.ceil["copy"] / 1e12, "read_TBps": b.ceil["read"] / 1e12, "read_no_store_TBps": b.ceil["read_probe"] / 1e12,
            "write_TBps": b.ceil["write"] / 1e12,
            "how": "xHipMemCeilingDev on the headline input / output buffers (%d MiB), trimmed mean of the timed launches' HIP-event durations, slowest rank: "
                   "nontemporal 16 B/lane streams in the launch shape that measured fastest for each (copy = the transform kernels' pattern, read = one XOR "
                   "checksum per 2 KiB, read_no_store = the same loads with nothing flowing back, write = the intra predictor's pattern)" % (ceil_bytes >> 20)}


def traffic_of_headline(b):
    """(pmc dict, source text): HBM bytes per launch from the counters -- measured live at N = 1, else replayed from profiles/traffic.json"""
    pmc, pmc_src = {}, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath) and b.n_dct == DCT_BLOCKS_PER_GPU and b.n_satd == SATD_BLOCKS_PER_GPU:
        try:
            pmc = json.load(open(tpath))
            pmc_src = "replayed from %s (builder's rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command); not measured in this run" % pmc.get("_source", "profiles/traffic.json")
        except Exception:
            pmc = {}
    if b.world == 1 and not b.args.no_live_traffic:
        b.hip.device_sync()
        live, how = measure_traffic_live(b.n_dct)
        if live is not None:
            pmc = dict(pmc, dct32_fwd_bytes_per_launch=live)
            pmc_src = how
        elif pmc_src:
            pmc_src += " (live passes: %s)" % how
        else:
            pmc_src = "not measured: " + how
    return pmc, pmc_src

# ------------------------------------------------------------------------------------------------
# the line the driver parses: compact (<= 4 KB), numbers only; the full record goes to bench_full.json
# ------------------------------------------------------------------------------------------------
COMPACT_LIMIT_BYTES = 4096             # target; tests/test_bench_line.py fails the build at 8192
FULL_RECORD = "bench_full.json"
_FRAC_KEYS = ("frac", "hbm_frac", "written_hbm_frac", "frac_of_v_sad_u16_floor", "frac_of_v_sad_u8_floor", "autotuned_hbm_frac")
_RATE_KEYS = ("value", "frames_per_s", "blocks_per_s", "ms_per_frame")
_GROUPS = ("transform_set", "classes", "per_ctu_mixed", "fused_from_tiles", "front_end_and_sad")   # containers, not legs: children keep their own names


def _sig(v, digits=5):
    """numbers of the compact line: 5 significant digits (ints and bools untouched)"""
    if isinstance(v, bool) or not isinstance(v, float):
        return v
    return float("%.*g" % (digits, v))


def _leg_scalars(name, leg, out, failed):
    """one leg of `also` -> {name: roofline fraction (else its rate)}; every boolean check of the leg must be true"""
    if not isinstance(leg, dict):
        return
    roof = leg.get("roofline") if isinstance(leg.get("roofline"), dict) else {}
    for k in _FRAC_KEYS:
        if isinstance(roof.get(k, leg.get(k)), (int, float)):
            out[name] = _sig(float(roof.get(k, leg.get(k))), 4)
            break
    else:
        for k in _RATE_KEYS:
            if isinstance(leg.get(k), (int, float)) and not isinstance(leg.get(k), bool):
                out[name] = _sig(float(leg[k]), 4)
                break
    for k, v in leg.items():
        if isinstance(v, bool) and k != "torch_imported" and not v:
            failed.append("%s.%s" % (name, k))
        elif isinstance(v, dict) and k not in ("roofline", "cpu_baseline", "pcie_link", "link_GBps"):
            _leg_scalars(k if name in _GROUPS else "%s.%s" % (name, k), v, out, failed)


def compact_record(full):
    """The single stdout line: the contract's top-level keys, `roofline` and `cpu_baseline` as numbers only, `also` as
    {leg: fraction-or-rate} scalars.  Everything else (notes, per-leg timing, how-it-was-measured prose) stays in the
    full record (FULL_RECORD, also on stderr).  BENCH_r05 failed to parse at 20 KB; this is held under 4 KB by test."""
    top = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
           "vs_baseline", "dtype", "data")
    line = {k: full.get(k) for k in top}                                # the contract's own numbers: full precision
    cfg = full.get("config", {})
    line["config"] = {"workload": "BASELINE configs[1]: batched 32x32 forward DCT, %d int16 residual blocks per GPU resident in HBM"
                                  % cfg.get("blocks_per_gpu", 0),
                      "blocks_per_gpu": cfg.get("blocks_per_gpu"), "block_bytes_in_plus_out": cfg.get("block_bytes_in_plus_out"),
                      "sharding": cfg.get("sharding")}
    r = full.get("roofline") or {}
    line["roofline"] = {k: _sig(r.get(k)) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms_per_launch",
                                                     "kernel_ms_mean", "algorithmic_bytes_per_launch", "frac_of_same_box_copy", "frac_at_mean")}
    if isinstance(r.get("traffic"), (int, float)):
        line["roofline"]["traffic"] = int(round(r["traffic"]))          # bytes per launch from the counters: whole bytes, next to the algorithmic count
    line["roofline"]["traffic_measured_live"] = "measured in this run" in str(r.get("traffic_source"))   # else replayed from profiles/traffic.json, or null
    if r.get("frac_by_rank"):
        line["roofline"]["frac_by_rank"] = [_sig(v, 4) for v in r["frac_by_rank"]]
    c = full.get("cpu_baseline")
    line["cpu_baseline"] = None if not c else {k: _sig(c.get(k)) for k in ("value", "unit", "cores", "kind", "single_thread_blocks_per_s",
                                                                             "host_cpu", "gpu_output_bit_exact_vs_cpu")}
    if c:
        line["cpu_baseline"]["sample"] = "all %d blocks of the GPU batch, same inputs, %s pinned threads" % (cfg.get("blocks_per_gpu", 0), c.get("cores"))
    if "secondary" in full:
        line["secondary"] = {k: _sig(v) for k, v in full["secondary"].items()}
    also, failed = {}, []
    for name, leg in (full.get("also") or {}).items():
        if name.endswith("_error") and name != "node_layer_error":      # a leg that threw (N = 1): named, the rest of the line stands
            failed.append(name)
        _leg_scalars(name, leg, also, failed)
    one = ((full.get("also") or {}).get("host_api") or {}).get("one_block_call_us")
    if one is not None:
        also["host_api.one_block_call_us"] = _sig(float(one), 4)
    if full.get("also") is not None:
        line["also"] = also
        line["checks_failed"] = failed
        if full["also"].get("node_layer_error"):
            line["node_layer_error"] = str(full["also"]["node_layer_error"])[:200]
        if full["also"].get("rccl_by_rank"):
            line["rccl_ranks"] = len(full["also"]["rccl_by_rank"])
    line["output_checksum_sum_i16"] = full.get("output_checksum_sum_i16")
    line["device"] = full.get("device")
    line["full_record"] = FULL_RECORD
    if "error" in full:
        line["error"] = full["error"]
    return line


def _finite(o):
    """NaN / +-Infinity are not JSON: a leg that divided by zero must cost its own scalar (null), never the line"""
    if isinstance(o, float):
        return o if o == o and o not in (float("inf"), float("-inf")) else None
    if isinstance(o, dict):
        return {k: _finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_finite(v) for v in o]
    return o


def emit(result, json_fd):
    """rank 0: the full record to FULL_RECORD (cwd; also gpurun_out/ when it exists), the compact line -- alone -- to stdout.
    stderr only gets a pointer: a consumer that reads both streams must not find a 20 KB line after the compact one."""
    full = json.dumps(_finite(result))
    for path in (FULL_RECORD, os.path.join("gpurun_out", FULL_RECORD) if os.path.isdir("gpurun_out") else None):
        if path:
            try:
                with open(path, "w") as f:
                    f.write(full + "\n")
            except OSError as e:
                sys.stderr.write("bench.py: could not write %s: %s\n" % (path, e))
    sys.stderr.write("bench.py: full record (%d bytes) in %s\n" % (len(full), os.path.abspath(FULL_RECORD)))
    sys.stderr.flush()
    os.write(json_fd, (json.dumps(_finite(compact_record(result)), separators=(",", ":"), allow_nan=False) + "\n").encode())


def spawn_ranks(args):
    """plain `python bench.py --gpus N`: become the launcher -- the command line the driver uses, one rank per GPU; torchrun picks and
    HOLDS the rendezvous port itself (--standalone: no bind-close-reuse race); rank 0's JSON line goes to this
    process's stdout, the exit status is the job's"""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    raise SystemExit(subprocess.call(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1")))


DUMP_BLOCKS, DUMP_SEED = 8192, 0x266D


def dump_outputs(b, z, out_dir):
    """the headline's output of its last step, as a caller would receive it (int16 coefficients, here as float32): a fixed, seeded
    sample of blocks in block order, copied block by block from the device (the whole batch is 2 GiB)"""
    n = min(DUMP_BLOCKS, b.n_dct)
    blocks = np.sort(np.random.default_rng(DUMP_SEED).choice(b.n_dct, n, replace=False))
    out = np.empty((n, 1024), np.int16)
    for i, blk in enumerate(blocks):
        b.codec._check(b.codec.L.xHipMemcpyD2H(b.codec.ctx, out[i].ctypes.data, z.ptr + int(blk) * 2048, 2048), "xHipMemcpyD2H")
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "dct32_fwd_coefficients.npy"), out.astype(np.float32))


def headline(b, x, z, same_box):
    head = b.timed_leg(lambda: b.codec.dct32_fwd_dev(x.ptr, z.ptr, b.n_dct, b.stream))
    if b.args.dump_outputs and b.rank == 0:
        dump_outputs(b, z, b.args.dump_outputs)
    pmc, pmc_src = traffic_of_headline(b) if b.args.full else ({}, None)
    result = {
        "metric": "dct32_fwd_blocks_per_s", "value": b.rate(head, b.n_dct), "unit": "blocks/s", "n_gpus": b.world,
        "steps": b.K, "warmup": b.W, "ms_per_step": head["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "i32", "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: batched 32x32 forward DCT, %d random 9-bit residual blocks per GPU "
                               "resident in HBM (with --full: inverse, fused fwd+inv, 8x8 SATD and the other configs under 'also')" % b.n_dct,
                   "blocks_per_gpu": b.n_dct, "block_bytes_in_plus_out": DCT_BYTES_PER_BLOCK,
                   "arithmetic": "int16 data as two int8 planes x int8 coefficients on v_mfma_i32_32x32x32_i8, int32 accumulate",
                   "sharding": "contiguous shard per rank, no data-path collective",
                   "clock_prewarm_launches": head["clock_prewarm_launches"],
                   "timing": "every leg: own clock pre-warm, W warm-up launches, K launches barrier-to-barrier; kernel_ms = 10 % trimmed mean of the HIP-event "
                             "durations recorded on the launching stream around those same K launches (mean and median next to it)"},
        "roofline": b.roofline(head, DCT_BYTES_PER_BLOCK, b.n_dct, pmc.get("dct32_fwd_bytes_per_launch"), pmc_src),
        "hip_runtime": {"version": b.hip.version(), "path": b.hip.paths[0], "copies_in_process": len(loaded_libraries("libamdhip64.so")),
                        "torch_imported": "torch" in sys.modules},
    }
    result["roofline"]["same_box"] = same_box
    return result, pmc, pmc_src


def main():
    args = parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.traffic_child:
        traffic_child(args)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)
    # stdout carries exactly ONE line, the JSON: libraries that chat on stdout (RCCL prints a version banner
    # when a communicator is created) are sent to stderr for the duration of the run
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    b = Bench(args)
    rank, world, codec = b.rank, b.world, b.codec

    # ---- inputs resident in HBM: this rank's slice of the one seeded stream -----------------
    x, z = b.dev(b.n_dct * 2048), b.dev(b.n_dct * 2048)
    codec.fill_residual_dev(x.ptr, b.n_dct * 1024, DCT_SEED, rank * b.n_dct * 1024, b.stream)
    b.hip.device_sync()
    same_box = leg_same_box(b, x, z) if args.full else None
    result, pmc, pmc_src = headline(b, x, z, same_box)
    result["output_checksum_sum_i16"] = None
    if args.full:
        # ---- checksum of the forward output across ranks (validates the sharded run) ----------------
        z_host = z.download(np.int16, b.n_dct * 1024)
        result["output_checksum_sum_i16"] = b.sum_over_ranks_i64(int(z_host.astype(np.int64).sum()))

    if args.full and not args.no_also:
        also, me = {}, {}

        def leg(name, fn, merge=False):
            """one family of `also`.  At N = 1 a leg that throws costs its own entry ("<name>_error", listed under checks_failed), not the line;
            with several ranks the exception stands: the other ranks are inside the leg's barriers and the launcher must end the job."""
            try:
                r = fn()
            except Exception as e:                                          # noqa: BLE001
                if world > 1:
                    raise
                also[name + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                return
            if merge:
                also.update(r)
            else:
                also[name] = r
        leg("dct32_inverse_and_fused", lambda: leg_dct32_inverse_and_fused(b, x, z, pmc, pmc_src), merge=True)
        leg("satd8x8", lambda: leg_satd(b, pmc, pmc_src))
        if not args.no_me:
            leg("motion_search", lambda: leg_motion_search(b, me), merge=True)
        if not args.no_transform_set:
            leg("transform_set", lambda: leg_transform_set(b, x))
            leg("fused_from_tiles", lambda: leg_fused_from_tiles(b))
            leg("front_end_and_sad", lambda: leg_front_end_and_sad(b))
            leg("intra32", lambda: leg_intra(b))
            if not args.no_autotune:
                leg("autotune", lambda: leg_autotuned(b, x, z))
        if rank == 0 and world == 1 and not args.no_host_api:
            leg("host_api", lambda: leg_host_api(b, min(b.n_dct, 1 << 17)))
        result["also"] = also
        if "satd8x8" in also:
            result["secondary"] = {"metric": "satd8x8_blocks_per_s", "value": also["satd8x8"]["value"], "unit": "blocks/s",
                                   "roofline_frac": also["satd8x8"]["roofline"]["frac"],
                                   "frac_of_same_box_read": also["satd8x8"]["roofline"]["frac_of_same_box_read"]}
        if (not b.share or os.environ.get("X266HIP_RCCL_LIB")) and args.stream8k > 0:
            run_node_legs_under_watchdog(b, result, also, x, z, me, json_fd, emit)
        also["rccl_libraries_in_process"] = loaded_libraries("librccl")

    # ---- CPU baseline for the headline leg (rank 0, N = 1 only) ------------------------------------
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        try:
            x_host = x.download(np.int16, b.n_dct * 1024).reshape(b.n_dct, 1024)
            base, exact = cpu_baseline_dct(x_host, z_host.reshape(b.n_dct, 1024))
            result["cpu_baseline"] = base
            if not exact:
                result["error"] = "GPU output differs from the CPU reference"
        except Exception as e:                                              # noqa: BLE001  (e.g. the checker's .so files did not travel: say so, keep the line)
            result["cpu_baseline"] = None
            result["error"] = "cpu_baseline leg failed: %s: %s" % (type(e).__name__, str(e)[:200])
    elif rank == 0:
        result["cpu_baseline"] = None

    if rank == 0:
        result["device"] = b.info["name"].strip()
        sys.stdout.flush()
        emit(result, json_fd)
    if b.dist is not None:
        if result.get("also", {}).get("node_layer_error"):               # peers may be stuck in a collective this rank left: no orderly shutdown
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        b.dist.destroy_process_group()
        # the library brought ROCm's HIP runtime, torch (control plane) was imported after it and bundles a second copy under the same SONAME: leave without
        # running two sets of exit handlers over one runtime's state (a CPU session in that import order ended in "double free or corruption" at exit)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
