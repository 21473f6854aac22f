#!/usr/bin/env python3
"""Timing of mixed inter / intra coding of a frame (xDct32CodeMixedFrameGpu) at 3840 x 2176, device events after warm-up, all in ONE
process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  xDct32CodeCtuTilesGpu     every region inter, one launch: what a P-frame costs without the fall-back
  xIntra32CodeFrameGpu      every region intra, 4 ctus_x + 6 ctus_y - 6 dependent launches
  mixed, every kind 0       one launch for the regions, then the steps, in which every workgroup returns after reading its kind byte:
                            the cost of the EMPTY steps is this leg minus the first launch
  mixed, every kind 1       the intra frame through the new kernels
  mixed, every kind 2       both costs for every region, then the cheaper prediction
  mixed, 5 % marked 2       a screened P-frame: a seeded 5 % of the CTUs decide (all six regions), the rest are given as inter
  each of these             plain on a created stream, and captured into a graph once and replayed

Reported per leg: time per call and time per step.  No rate is a pass / fail condition.
The frame is the "oriented" recipe of tests/_intra_frame_ref.py at frame size; the inter prediction is the frame plus +-6 noise, and
255 - the frame in every other 32x32 block (motion compensation that failed there), as in tests/_mixed_frame_ref.py.
Usage: gpu_mixed_frame.py [--out FILE]   (default profiles/r22_mixed_frame.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from gpu_intra_frame import frame, tiles_of, trimmed_mean  # noqa: E402

ROUNDS, REPS, QP, ROUNDING, PENALTY = 12, 3, 27, 171, 64


def measure(codec, w, h, say):
    n, tile_bytes = codec.ctu_count(w, h), w * h * 2
    steps = 4 * (w // 64) + 6 * (h // 64) - 6
    rs = np.random.RandomState(0x266)
    planes = frame(rs, w, h)
    failed = [((np.mgrid[0:p.shape[0], 0:p.shape[1]] // 32).sum(axis=0) & 1).astype(bool) for p in planes]
    pred_planes = [np.where(f, 255 - p, np.clip(p.astype(np.int64) + rs.randint(-6, 7, p.shape), 0, 255)).astype(np.uint8) for p, f in zip(planes, failed)]
    cur, pred, recon = codec.alloc(tile_bytes), codec.alloc(tile_bytes), codec.alloc(tile_bytes)
    level, nnz, kind, mode, cost = codec.alloc(n * 12288), codec.alloc(n * 24), codec.alloc(n * 6), codec.alloc(n * 6), codec.alloc(n * 48)
    cur.upload(tiles_of(*planes, rs))
    pred.upload(tiles_of(*pred_planes, rs))
    recon.upload(np.zeros(tile_bytes, np.uint8))
    screened = np.zeros((n, 6), np.uint8)
    screened[rs.permutation(n)[:max(1, n // 20)]] = 2
    kinds = {"every kind 0": np.zeros((n, 6), np.uint8), "every kind 1": np.ones((n, 6), np.uint8), "every kind 2": np.full((n, 6), 2, np.uint8),
             "5 % marked 2": screened}
    d_kinds = {}
    for k, a in kinds.items():
        d_kinds[k] = codec.alloc(n * 6)
        d_kinds[k].upload(a)
    st = codec.stream_create()
    ev = [codec.event_create() for _ in range(2)]

    def mixed(k):
        p = codec.mixed_params(w, h, QP, ROUNDING, PENALTY, d_cur=cur.ptr, d_pred=pred.ptr, d_kind_in=d_kinds[k].ptr, d_level=level.ptr, d_nnz=nnz.ptr,
                               d_kind=kind.ptr, d_mode=mode.ptr, d_cost=cost.ptr, d_recon=recon.ptr)
        return lambda: codec.dct32_code_mixed_frame_dev(p, stream=st)

    calls = {"xDct32CodeCtuTilesGpu": lambda: codec.dct32_code_ctu_tiles_dev(cur.ptr, pred.ptr, w, h, 0, QP, ROUNDING, level.ptr, nnz.ptr, recon.ptr, stream=st),
             "xIntra32CodeFrameGpu": lambda: codec.intra32_code_frame_dev(cur.ptr, w, h, 0, QP, ROUNDING, 0, level.ptr, nnz.ptr, mode.ptr, recon.ptr, stream=st)}
    for k in kinds:
        calls["mixed, " + k] = mixed(k)

    # what the legs code: the two ends are the existing calls' bits (the tests hold the statement), the others are counted
    def coded(k):
        calls[k]()
        codec.stream_sync(st)
        return level.download(np.int16, n * 6144), recon.download(np.uint8, tile_bytes), kind.download(np.uint8, n * 6)

    inter, intra = coded("xDct32CodeCtuTilesGpu"), coded("xIntra32CodeFrameGpu")
    for k, ref in (("mixed, every kind 0", inter), ("mixed, every kind 1", intra)):
        got = coded(k)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].reshape(-1, 512)[:, :384], ref[1].reshape(-1, 512)[:, :384]), k
    say("\n%d x %d (%d CTUs, %d regions, %d steps), qp %d, intra_penalty %d" % (w, h, n, 6 * n, steps, QP, PENALTY))
    for k in ("every kind 2", "5 % marked 2"):
        got = coded("mixed, " + k)[2].reshape(n, 6)
        deciding = int((kinds[k][:, :5] == 2).sum())
        say("  %-14s %6d of %d regions decide (U and V as one), %d of them end intra" % (k + ":", deciding, 5 * n, int(got[:, :5][kinds[k][:, :5] == 2].sum())))

    graphs = {}
    for k in list(calls):
        codec.graph_begin(st)
        calls[k]()
        graphs[k] = codec.graph_end(st)
        calls[k + ", graph"] = lambda g=graphs[k]: codec.graph_launch(g, st)

    def timed(k):
        reps = 20 * REPS if k.startswith("xDct32CodeCtuTilesGpu") else REPS
        codec.event_record(ev[0], st)
        for _ in range(reps):
            calls[k]()
        codec.event_record(ev[1], st)
        codec.stream_sync(st)
        return codec.event_elapsed_ms(ev[0], ev[1]) / reps

    for fn in calls.values():                                               # warm-up: code objects, clocks
        fn()
    codec.stream_sync(st)
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds, all legs alternating (%d calls per round for the stepped calls, %d for the one-launch call)" % (ROUNDS, REPS, 20 * REPS))
    say("%-36s %10s %10s %10s %10s" % ("leg", "us", "min us", "max us", "us / step"))
    for k in calls:
        per_step = "" if k.startswith("xDct32CodeCtuTilesGpu") else "%10.2f" % (t[k] * 1e3 / steps)
        say("%-36s %10.1f %10.1f %10.1f %10s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, per_step))
    for suffix in ("", ", graph"):
        empty = (t["mixed, every kind 0" + suffix] - t["xDct32CodeCtuTilesGpu" + suffix]) * 1e3
        say("an empty step%s: (mixed, every kind 0 - xDct32CodeCtuTilesGpu) / %d steps = %.2f us; the screened frame is %.2f x the intra frame's time, "
            "%.2f x the inter frame's" % (suffix, steps, empty / steps, t["mixed, 5 % marked 2" + suffix] / t["xIntra32CodeFrameGpu" + suffix],
                                          t["mixed, 5 % marked 2" + suffix] / t["xDct32CodeCtuTilesGpu" + suffix]))
    for g in graphs.values():
        codec.graph_free(g)
    for e in ev:
        codec.event_destroy(e)
    codec.stream_destroy(st)


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r22_mixed_frame.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    say("device: %s" % (codec.device_info(),))
    measure(codec, 3840, 2176, say)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
