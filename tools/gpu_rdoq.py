#!/usr/bin/env python3
"""Timing of rate-distortion optimised quantisation and of the level rate estimate (xRdoQuantRegionsGpu, xLevelsBitsGpu) beside the
plain quantiser xQuantRegionsGpu(0) as the yardstick, on the same buffers: device events after warm-up, all in ONE process, the legs
alternating within every round, 10 % trimmed mean over the rounds.

  12 240 regions     the coefficients of one 3840 x 2176 4:2:0 frame (xDct32FwdCtuFromTilesDev of the me_frames pair of tests/_util.py:
                     a smooth picture, its displaced and noisy copy as the prediction), 25 MB in and 25 MB out: cache resident
  257 040 regions    that frame's coefficients 21 times over, 526 MB in and 526 MB out: larger than the 256 MB last-level cache

Both at qp 32, lambda 368, rounding 171, d_class and d_qp NULL (every region 32x32).  xLevelsBitsGpu reads the plain quantiser's
levels.  "x quant" = call time / the yardstick's time; "GB/s" = the bytes the call must move (in + out; the estimate: in) / call time.
No rate is a pass / fail condition.

Then host/rdoq_example (1920 x 1088, qp 32): plain quantiser at rounding 171 against lambda 368 -- non-zero levels, estimated bits,
packed stream words, squared error of the reconstruction.  The estimate is the static rate model's own; no bitrate is claimed.
Usage: gpu_rdoq.py [--out FILE]   (default profiles/r23_rdoq.txt)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from gpu_levels import frame_pair, trimmed_mean  # noqa: E402

ROUNDS, QP, LAMBDA, ROUNDING = 20, 32, 368, 171


def measure(codec, ev, coef_host, copies, reps, say):
    n = coef_host.shape[0] * copies
    nbytes = n * 2048
    coef, level, plain, nnz, stat = codec.alloc(nbytes), codec.alloc(nbytes), codec.alloc(nbytes), codec.alloc(4 * n), codec.alloc(16 * n)
    for i in range(copies):
        codec._check(codec.L.xHipMemcpyH2D(codec.ctx, coef.ptr + i * coef_host.nbytes, coef_host.ctypes.data, coef_host.nbytes), "xHipMemcpyH2D")
    p_rdoq = codec.rdoq_params(coef.ptr, level.ptr, 0, 0, nnz.ptr, stat.ptr, n, QP, LAMBDA)
    p_bits = codec.rdoq_params(0, plain.ptr, 0, 0, 0, stat.ptr, n)
    calls = {"xQuantRegionsGpu(0)": (lambda: codec.quant_regions_dev(0, coef.ptr, plain.ptr, n, 0, 0, QP, ROUNDING, nnz.ptr), 2 * nbytes),
             "xRdoQuantRegionsGpu": (lambda: codec.rdo_quant_dev(p_rdoq), 2 * nbytes),
             "xLevelsBitsGpu": (lambda: codec.levels_bits_dev(p_bits), nbytes)}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(reps):
            calls[k][0]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / reps

    for fn, _ in calls.values():                                        # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("\n%d regions (%.0f MB in, %.0f MB out), qp %d, lambda %d, rounding %d: 10 %% trimmed mean of %d rounds of %d calls, all legs alternating"
        % (n, nbytes / 1e6, nbytes / 1e6, QP, LAMBDA, ROUNDING, ROUNDS, reps))
    say("%-24s %10s %10s %10s %9s %9s" % ("call", "us", "min us", "max us", "x quant", "GB/s"))
    for k in calls:
        say("%-24s %10.2f %10.2f %10.2f %9.2f %9.0f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, t[k] / t["xQuantRegionsGpu(0)"],
                                                       calls[k][1] / (t[k] * 1e-3) / 1e9))
    return t


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r23_rdoq.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    example = subprocess.run([os.path.join(ROOT, "host", "rdoq_example"), "1920", "1088", str(QP), str(LAMBDA)], capture_output=True, text=True, timeout=120)
    if example.returncode != 0:
        raise SystemExit("host/rdoq_example failed: %s" % example.stderr[-2000:])
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    w, h = 3840, 2176
    cur, pred = frame_pair(codec, w, h)
    n = 6 * codec.ctu_count(w, h)
    coef = codec.alloc(n * 2048)
    codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred.ptr, w, h, coef.ptr)
    codec.stream_sync()
    coef_host = coef.download(np.int16, n * 1024).reshape(n, 1024)
    del coef, cur, pred
    measure(codec, ev, coef_host, 1, 20, say)
    measure(codec, ev, coef_host, 21, 3, say)
    for e in ev:
        codec.event_destroy(e)
    r = json.loads(example.stdout.strip().splitlines()[-1])
    say("\nhost/rdoq_example, %s, qp %d, %d regions: plain quantiser at rounding 171 against lambda %d" % (r["frame"], r["qp"], r["regions"], r["lambda"]))
    say("%-8s %16s %18s %14s %16s" % ("", "non-zero levels", "estimated bits", "stream words", "SSE of recon"))
    for k in ("plain", "rdoq"):
        say("%-8s %16d %18.1f %14d %16d" % (k, r[k]["nonzero_levels"], r[k]["estimated_bits"], r[k]["stream_words"], r[k]["sse"]))
    say("rdoq / plain %13.3f %18.3f %14.3f %16.3f" % tuple(r["rdoq"][f] / max(r["plain"][f], 1) for f in ("nonzero_levels", "estimated_bits", "stream_words", "sse")))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
