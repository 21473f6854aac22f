#!/usr/bin/env python3
"""Timing of the transform decision (xTransformDecideCtuTilesGpu) beside the composition it replaces -- per candidate class
xTransformCtuFromTilesDev with every class byte equal to it, then xRdoQuantRegionsGpu with d_stat -- on the same buffers: device events
after warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds.  The composition is timed
WITHOUT the step that picks each region's winner and gathers its levels (no device call does that): it is a lower bound of what the
call replaces.

  12 240 regions     one 3840 x 2176 4:2:0 frame (the me_frames pair of tests/_util.py: a smooth picture, its displaced and noisy copy
                     as the prediction), qp 32, lambda 368, no side bits, d_qp and d_cand NULL; with all 13 candidates and with the
                     DCT-II four (mask 0x000F)

"spread" = (max - min) / trimmed mean over a leg's rounds.  The verdict line says whether the call is faster than the composition by
more than the run-to-run spread: its slowest round against the composition's fastest.  No ratio is a pass / fail condition.

Then host/tdecide_example (1920 x 1088, qp 32, lambda 368): the class histogram and, against the all-32x32 xRdoQuantRegionsGpu chain at
the same lambda, summed J, estimated bits, packed words and the squared error of the actual reconstruction; and the ratio of the
summed dist, scaled by Qstep^2, to that squared error -- how far the coefficient-domain distortion is from the sample domain.  The
estimate is the static rate model's own; no bitrate is claimed.
Usage: gpu_tdecide.py [--out FILE]   (default profiles/r24_tdecide.txt)"""
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

ROUNDS, REPS, QP, LAMBDA = 20, 3, 32, 368
MASKS = (("all 13 candidates", 0x777F), ("the DCT-II four", 0x000F))


def measure(codec, ev, w, h, say):
    cur, pred = frame_pair(codec, w, h)
    n = 6 * codec.ctu_count(w, h)
    cls, level, nnz, stat, cost = codec.alloc(n), codec.alloc(n * 2048), codec.alloc(4 * n), codec.alloc(16 * n), codec.alloc(128 * n)
    coef, lvl2 = codec.alloc(n * 2048), codec.alloc(n * 2048)
    tabs = {}
    for k in range(15):
        tabs[k] = codec.alloc(n)
        tabs[k].upload(np.full(n, k, np.uint8))
    legs = {}
    for name, mask in MASKS:
        p = codec.tdecide_params(cur.ptr, pred.ptr, 0, 0, cls.ptr, level.ptr, nnz.ptr, stat.ptr, cost.ptr, w, h, QP, LAMBDA, mask, mask)
        legs["the call, " + name] = (lambda p=p: codec.transform_decide_dev(p))

        def composition(mask=mask):
            for k in range(15):
                if (mask >> k) & 1:
                    codec.transform_ctu_from_tiles_dev(cur.ptr, pred.ptr, w, h, tabs[k].ptr, coef.ptr)
                    codec.rdo_quant_dev(codec.rdoq_params(coef.ptr, lvl2.ptr, tabs[k].ptr, 0, nnz.ptr, stat.ptr, n, QP, LAMBDA))
        legs["composition, " + name] = composition

    def timed(fn):
        codec.event_record(ev[0])
        for _ in range(REPS):
            fn()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in legs.values():                                            # warm-up: code objects, clocks
        for _ in range(2):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("\n%d regions of %d x %d, qp %d, lambda %d: 10 %% trimmed mean of %d rounds of %d calls, all legs alternating" % (n, w, h, QP, LAMBDA, ROUNDS, REPS))
    say("%-36s %10s %10s %10s %9s %14s" % ("leg", "us", "min us", "max us", "spread", "ns / region"))
    for k in legs:
        say("%-36s %10.1f %10.1f %10.1f %8.1f%% %14.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, 100 * (max(ms[k]) - min(ms[k])) / t[k],
                                                         t[k] * 1e6 / n))
    for name, _ in MASKS:
        a, b = "the call, " + name, "composition, " + name
        beyond = max(ms[a]) < min(ms[b])
        say("%s: the call takes %.3f of the composition's time; %s" % (name, t[a] / t[b], "faster by more than the run-to-run spread (its slowest round %.1f us "
            "against the composition's fastest %.1f us)" % (max(ms[a]) * 1e3, min(ms[b]) * 1e3) if beyond else
            "NOT faster by more than the run-to-run spread (its slowest round %.1f us, the composition's fastest %.1f us)" % (max(ms[a]) * 1e3, min(ms[b]) * 1e3)))
    return t


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r24_tdecide.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    example = subprocess.run([os.path.join(ROOT, "host", "tdecide_example"), "1920", "1088", str(QP), str(LAMBDA)], capture_output=True, text=True, timeout=120)
    if example.returncode != 0:
        raise SystemExit("host/tdecide_example failed: %s" % example.stderr[-2000:])
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    measure(codec, ev, 3840, 2176, say)
    for e in ev:
        codec.event_destroy(e)
    r = json.loads(example.stdout.strip().splitlines()[-1])
    say("\nhost/tdecide_example, %s, qp %d, lambda %d, %d regions, all 13 candidates, made-up side bits" % (r["frame"], r["qp"], r["lambda"], r["regions"]))
    say("class histogram (class byte: regions): " + ", ".join("%d: %d" % (k, c) for k, c in enumerate(r["class_histogram"]) if c))
    fields = ("sum_j_without_side_bits", "estimated_bits", "nonzero_levels", "stream_words", "sse")
    say("%-10s %18s %16s %16s %14s %16s" % ("", "summed J", "estimated bits", "non-zero levels", "stream words", "SSE of recon"))
    for k in ("all_dct32", "decided"):
        say("%-10s %18d %16.1f %16d %14d %16d" % ((k,) + tuple(r[k][f] for f in fields)))
    say("decided / all_dct32 %9.3f %16.3f %16.3f %14.3f %16.3f" % tuple(r["decided"][f] / max(r["all_dct32"][f], 1) for f in fields))
    qstep2 = 2.0 ** ((r["qp"] - 4) / 3.0)
    for k in ("all_dct32", "decided"):
        say("%s: summed dist / 65536 * Qstep^2 = %.0f, %.3f of the squared error of the reconstruction" % (k, r[k]["sum_dist"] / 65536.0 * qstep2,
                                                                                                        r[k]["sum_dist"] / 65536.0 * qstep2 / max(r[k]["sse"], 1)))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
