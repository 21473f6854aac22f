#!/usr/bin/env python3
"""Timing of intra coding on tiled frames at 1920 x 1088 and 3840 x 2176 (the calls take multiples of 64), device events after
warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  closed loop          xIntra32CodeFrameGpu with the mode decision: one launch per step, 4 ctus_x + 6 ctus_y - 6 steps
  modes given          the same call with d_mode_in (the decided modes): no decision
  open-loop front      xIntra32RefsFromTilesGpu on the SOURCE frame's luma + xIntra32CostsDev over its 4 n_ctu blocks
  each of these        plain on a created stream, and captured into a graph once and replayed
  for scale            xDct32CodeCtuTilesGpu on the same frame (pred = the closed loop's reconstruction): the fully parallel coding call

Reported per leg: time per call, and for the two frame calls the time per step.  No rate is a pass / fail condition.
The frame is the "oriented" recipe of tests/_intra_frame_ref.py at frame size: per 32x32 block a sinusoid at a block-dependent angle
plus +-4 noise, U the 2:1 mean of luma and V its complement.
Usage: gpu_intra_frame.py [--out FILE]   (default profiles/r15_intra_frame.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS, QP, ROUNDING = 12, 3, 27, 171


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def frame(rs, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    k = (yy // 32) * (w // 32) + xx // 32
    ang = np.pi * ((k * 7) % 16) / 16.0
    img = 128 + 90 * np.sin((xx * np.cos(ang) + yy * np.sin(ang)) * 0.35 + k)
    sub = img.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    noisy = lambda p: np.clip(p + rs.randint(-4, 5, p.shape), 0, 255).astype(np.uint8)
    return noisy(img), noisy(sub), noisy(255 - sub)


def tiles_of(y, u, v, rs):
    h, w = y.shape
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    c = np.stack([u, v], axis=-1).reshape(h // 16, 8, w // 16, 16).transpose(0, 2, 1, 3)
    t[:, :, 256:384] = c.reshape(h // 16, w // 16, 128)
    return t.ravel()


def measure(codec, w, h, say):
    n, tile_bytes = codec.ctu_count(w, h), w * h * 2
    steps = 4 * (w // 64) + 6 * (h // 64) - 6
    rs = np.random.RandomState(0x266)
    y, u, v = frame(rs, w, h)
    cur, recon, pred = codec.alloc(tile_bytes), codec.alloc(tile_bytes), codec.alloc(tile_bytes)
    level, nnz, mode, mode_in = codec.alloc(n * 12288), codec.alloc(n * 24), codec.alloc(n * 6), codec.alloc(n * 6)
    refs, costs, best = codec.alloc(4 * n * 144), codec.alloc(4 * n * 35 * 4), codec.alloc(4 * n)
    blocks = codec.alloc(4 * n * 1024)                                      # the luma blocks in the order of the sets, 1 KiB each, for xIntra32CostsDev
    cur.upload(tiles_of(y, u, v, rs))
    recon.upload(np.zeros(tile_bytes, np.uint8))
    blocks.upload(y.reshape(h // 64, 2, 32, w // 64, 2, 32).transpose(0, 3, 1, 4, 2, 5))
    st = codec.stream_create()
    ev = [codec.event_create() for _ in range(2)]

    calls = {"closed loop": lambda: codec.intra32_code_frame_dev(cur.ptr, w, h, 0, QP, ROUNDING, 0, level.ptr, nnz.ptr, mode.ptr, recon.ptr, stream=st),
             "modes given": lambda: codec.intra32_code_frame_dev(cur.ptr, w, h, 0, QP, ROUNDING, mode_in.ptr, level.ptr, nnz.ptr, mode.ptr, recon.ptr, stream=st)}

    def front():
        codec.intra32_refs_from_tiles_dev(cur.ptr, w, h, 0, refs.ptr, stream=st)
        codec.intra32_costs_dev(refs.ptr, blocks.ptr, costs.ptr, best.ptr, 4 * n, stream=st)
    calls["open-loop front"] = front

    # the decided modes feed the second leg; both legs give the same frame (the tests hold the statement)
    calls["closed loop"]()
    codec.stream_sync(st)
    decided = mode.download(np.uint8, n * 6)
    first = (level.download(np.int16, n * 6144), recon.download(np.uint8, tile_bytes))
    mode_in.upload(decided)
    pred.upload(first[1])
    calls["modes given"]()
    front()
    codec.stream_sync(st)
    assert np.array_equal(level.download(np.int16, n * 6144), first[0]) and np.array_equal(recon.download(np.uint8, tile_bytes), first[1]), \
        "the call with the decided modes differs from the closed loop"
    open_loop = best.download(np.uint8, 4 * n)
    luma = decided.reshape(n, 6)[:, :4].ravel()
    say("\n%d x %d (%d CTUs, %d steps), qp %d: %d distinct luma modes, %.1f %% of the open-loop decisions are the closed loop's, %.1f %% of the levels non-zero" % (
        w, h, n, steps, QP, len(set(luma.tolist())), 100.0 * (open_loop == luma).mean(), 100.0 * (first[0] != 0).mean()))

    graphs = {}
    for k in list(calls):
        codec.graph_begin(st)
        calls[k]()
        graphs[k] = codec.graph_end(st)
        calls[k + ", graph"] = lambda g=graphs[k]: codec.graph_launch(g, st)
    calls["xDct32CodeCtuTilesGpu"] = lambda: codec.dct32_code_ctu_tiles_dev(cur.ptr, pred.ptr, w, h, 0, QP, ROUNDING, level.ptr, nnz.ptr, recon.ptr, stream=st)

    def timed(k):
        reps = REPS if k.startswith(("closed", "modes")) else 20 * REPS
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
    say("10 %% trimmed mean of %d rounds, all legs alternating (%d calls per round for the frame calls, %d for the others)" % (ROUNDS, REPS, 20 * REPS))
    say("%-28s %10s %10s %10s %10s" % ("leg", "us", "min us", "max us", "us / step"))
    for k in calls:
        per_step = "%10.2f" % (t[k] * 1e3 / steps) if k.startswith(("closed", "modes")) else ""
        say("%-28s %10.1f %10.1f %10.1f %10s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, per_step))
    for g in graphs.values():
        codec.graph_free(g)
    for e in ev:
        codec.event_destroy(e)
    codec.stream_destroy(st)


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r15_intra_frame.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    say("device: %s" % (codec.device_info(),))
    for w, h in ((1920, 1088), (3840, 2176)):
        measure(codec, w, h, say)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
