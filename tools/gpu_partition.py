#!/usr/bin/env python3
"""Timing of the inter partition decision (xInterPartitionDecideGpu) at 3840 x 2176 (4K padded to whole CTUs), device events after warm-up,
all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  partition r = 0 / 1     the call alone, lambda_q4 64, with d_nodes: 1 + 4 * 3 = 13 and 1 + 36 * 3 = 109 scores per 8x8 block
  (a) refinement          xSatd8x8RefineQpelFromTilesGpu on the same pair: 49 scores per block, the known per-block-score yardstick
  (b) r = 0 / 1           what a host has to do today for the same scores: 1 + 12 (2r + 1)^2 pairs of xMotionCompQpelLumaGpu +
                          xSatd8x8FromTilesDev launches on prebuilt candidate fields (nine fields, the refined one moved by every (dx, dy) of
                          -1..1, taken in turn), WITHOUT the decision.  Unchanged code: its own baseline, not a threshold.

The field is the result of the lowres search + seeded search + refinement of tools/gpu_seeded.py on its frames (tests/_util.py's me_frames
pair, a smooth random picture and a copy moved by (11, -7) with noise).  The ratios to (a) and (b) are what is reported; no rate is a pass /
fail condition.  The decision at lambda_q4 64, r = 1 is recorded: partitions per level, the summed j against the unmerged field's summed Jw
(level-0 Jw from tests/_partition_ref.py's predictor and rate over the field and the refinement's own SATDs), and the output field is put
through xMotionCompQpelLumaGpu + xSatd8x8FromTilesDev and must return its own costs.  Nothing is claimed about bitrate; no lambda is tuned.
Usage: gpu_partition.py [--out FILE] [--size W H]   (default profiles/r27_partition.txt, 3840 2176)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.partition as P  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402

ROUNDS, REPS = 10, 3
LAMBDA = 64


def measure(codec, ev, w, h, say):
    import _partition_ref as R
    import _seeded_ref as S
    from _util import Oracle, me_frames
    oracle = Oracle()
    n, nb, n_ctu, nn = (w // 16) * (h // 16), (w // 8) * (h // 8), ((w + 63) // 64) * ((h + 63) // 64), P.node_count(w, h)
    cur, ref = me_frames(w, h, 0, 0x2121, mv=(11, -7))
    al = codec.alloc
    d = dict(cur=al(n * 512), ref=al(n * 512), low=al(n * 128), ref_low=al(n * 128), low_best=al(8 * n), best=al(8 * nb), q=al(8 * nb), q2=al(8 * nb), out=al(8 * nb),
             level=al(nb), ctu=al(16 * n_ctu), nodes=al(8 * nn), pred=al(n * 512), cost=al(4 * nb))
    d["cur"].upload(S.tiles_of(oracle, cur, 1))
    d["ref"].upload(S.tiles_of(oracle, ref, 2))
    d["pred"].upload(np.zeros(n * 512, np.uint8))
    for a, b in (("cur", "low"), ("ref", "ref_low")):
        codec.la_downscale_dev(codec.la_params(w, h, d_src=d[a].ptr, d_low=d[b].ptr))
    codec.satd_search_from_tiles_dev(d["low"].ptr, d["ref_low"].ptr, w // 2, h // 2, 32, d["low_best"].ptr)
    codec.satd_seeded_search_dev(codec.seed_params(w, h, 1, 31, 2, 16, d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_seed=d["low_best"].ptr, d_best=d["best"].ptr))
    refine = lambda dst="q": codec.satd_refine_qpel_from_tiles_dev(d["cur"].ptr, d["ref"].ptr, w, h, d["best"].ptr, d[dst].ptr)
    refine()
    codec.stream_sync()
    field = d["q"].download(np.uint8, 8 * nb).view(S.ME_DTYPE)
    part = {r: P.part_params(d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_mv=d["q"].ptr, d_out=d["out"].ptr, d_level=d["level"].ptr, d_ctu=d["ctu"].ptr,
                             d_nodes=d["nodes"].ptr, width=w, height=h, range=r, lambda_q4=LAMBDA) for r in (0, 1)}
    jitter = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            f = field.copy()
            f["mvx"] += dx
            f["mvy"] += dy
            jitter.append(codec._upload(f.view(np.uint8)))

    def pair(i):
        codec.motion_comp_qpel_luma_dev(d["ref"].ptr, jitter[i % 9].ptr, w, h, d["pred"].ptr)
        codec.satd8x8_from_tiles_dev(d["cur"].ptr, d["pred"].ptr, w, h, d["cost"].ptr)

    scores = {r: 1 + 12 * (2 * r + 1) ** 2 for r in (0, 1)}

    # one pass of the decision, checked
    say("\n%d x %d: %d blocks, %d CTUs, %d whole nodes; me_frames pair moved by (11, -7); the field of lowres + seeded + refinement" % (w, h, nb, n_ctu, nn))
    fin = R.field_in(np.stack([field["mvx"], field["mvy"]], axis=1), w, h)
    bw = w // 8
    jw0 = int(field["cost"].astype(np.int64).sum()) + sum(R.rate_cost(LAMBDA, R.rate(0, (int(fin[b // bw, b % bw, 0]), int(fin[b // bw, b % bw, 1])),
                                                                                  R.predictor(fin, b % bw, b // bw, 1))) for b in range(nb))
    for r in (0, 1):
        codec.inter_partition_decide_dev(part[r])
        codec.stream_sync()
        out, level = d["out"].download(np.uint8, 8 * nb).view(S.ME_DTYPE), d["level"].download(np.uint8, nb)
        ctu = d["ctu"].download(np.uint8, 16 * n_ctu).view(x266_amd.PART_CTU_DTYPE)
        codec.motion_comp_qpel_luma_dev(d["ref"].ptr, d["out"].ptr, w, h, d["pred"].ptr)
        codec.satd8x8_from_tiles_dev(d["cur"].ptr, d["pred"].ptr, w, h, d["cost"].ptr)
        codec.stream_sync()
        assert np.array_equal(d["cost"].download(np.uint32, nb), out["cost"]), "the output field does not reproduce its own costs"
        at = np.bincount(level, minlength=4)
        assert int(ctu["parts"].sum()) == sum(int(at[k]) >> (2 * k) for k in range(4)) and int(ctu["dist"].sum()) == int(out["cost"].sum())
        say("decision at lambda_q4 %d, r = %d: partitions per level %s (%d in all, of %d blocks); summed j %d against the unmerged field's summed Jw %d (%.3f); "
            "summed dist %d against its summed SATD %d; the output field returns its own costs through motion compensation + SATD"
            % (LAMBDA, r, [int(at[k]) >> (2 * k) for k in range(4)], int(ctu["parts"].sum()), nb, int(ctu["j"].sum()), jw0, int(ctu["j"].sum()) / jw0,
               int(ctu["dist"].sum()), int(field["cost"].astype(np.int64).sum())))
        assert int(ctu["j"].sum()) <= jw0

    calls = {"partition r = 0": lambda: codec.inter_partition_decide_dev(part[0]), "partition r = 1": lambda: codec.inter_partition_decide_dev(part[1]),
             "(a) refinement": lambda: refine("q2"), "(b) r = 0: 13 pairs": lambda: [pair(i) for i in range(scores[0])],
             "(b) r = 1: 109 pairs": lambda: [pair(i) for i in range(scores[1])]}
    per_block = {"partition r = 0": scores[0], "partition r = 1": scores[1], "(a) refinement": 49, "(b) r = 0: 13 pairs": scores[0], "(b) r = 1: 109 pairs": scores[1]}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in calls.values():                                           # warm-up: code objects, clocks
        for _ in range(2):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d back-to-back calls, all legs alternating; scores: 8x8 interpolations + SATDs per block" % (ROUNDS, REPS))
    say("%-24s %10s %10s %10s %8s %12s" % ("leg", "us", "min us", "max us", "scores", "Gscore/s"))
    for k in calls:
        say("%-24s %10.1f %10.1f %10.1f %8d %12.2f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, per_block[k], per_block[k] * nb / t[k] / 1e6))
    for r in (0, 1):
        p, b = t["partition r = %d" % r], t["(b) r = %d: %d pairs" % (r, scores[r])]
        say("r = %d: the call / (a) = %.2f with %.2f x its scores; the call / (b) = %.3f: the one call takes %s time than the %d launch pairs (%.1f x)"
            % (r, p / t["(a) refinement"], scores[r] / 49.0, p / b, "LESS" if p < b else "MORE", scores[r], b / p))
    say("accounting: a score of (b) reads a block's window and writes and re-reads 64 predicted bytes through memory, %d bytes of frames per pair;"
        " the call keeps the window rows and the scores in LDS and writes %d bytes per block once" % (3 * w * h * 2, 8 + 1))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r27_partition.txt")
    size = (3840, 2176)
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    if "--size" in argv:
        size = (int(argv[argv.index("--size") + 1]), int(argv[argv.index("--size") + 2]))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    measure(codec, ev, size[0], size[1], say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
