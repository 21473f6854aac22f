#!/usr/bin/env python3
"""Timing of the hierarchical motion search at 3840 x 2176 (4K padded to whole CTUs), device events after warm-up, all in ONE process, the
legs alternating within every round, 10 % trimmed mean over the rounds:

  (a) lowres + seeded   xSatd8x8SearchFromTilesDev at +-32 on the two half-size frames (= +-64 full-resolution samples), then
                        xSatd8x8SeededSearchGpu around the doubled winners: seed_scale 1, centres 31, r = 2, lambda_q4 16
  (b) exhaustive +-64   xSatd8x8SearchFromTilesDev at +-64 on the full-resolution pair: what (a) replaces
  lowres search         the first half of (a) alone
  seeded r = 0 / 2 / 8  the seeded call alone (seed_scale 1, centres 31, lambda_q4 16)
  seeded, per block     the seeded call with seed_scale 0 on the exhaustive search's own field (a previous field's form), r = 2
  downscale x 2         the two xLaDownscaleGpu calls in front of (a), for scale: a lookahead has made them already

(a) / (b) is the figure the call exists for; no rate is a pass / fail condition.  The frames are tests/_util.py's me_frames pair (a smooth
random picture and a copy moved by (11, -7) with noise).  The seeded winners are checked on the host: every winner's SATD is recomputed by
the oracle from the two planes, d_j = SATD + the vector cost of tests/_seeded_ref.py, and the agreement with the exhaustive field is
counted.
Usage: gpu_seeded.py [--out FILE]   (default profiles/r21_seeded_search.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402

ROUNDS, REPS = 12, 5


def check(oracle, cur, ref, seeds, scale, lam, best, j, say, what):
    """every winner's SATD recomputed from the planes; J = SATD + the vector cost against the block's own (clamped) seed"""
    import _seeded_ref as R
    h, w = cur.shape
    bw, nb = w // 8, (w // 8) * (h // 8)
    gw = R.grid(w, h, scale)[0]
    b = np.arange(nb)
    bx, by = b % bw, b // bw
    k = np.arange(8)
    ys = np.clip(8 * by[:, None] + best["mvy"].astype(np.int64)[:, None] + k, 0, h - 1)
    xs = np.clip(8 * bx[:, None] + best["mvx"].astype(np.int64)[:, None] + k, 0, w - 1)
    pred = ref[ys[:, :, None], xs[:, None, :]].astype(np.int16)
    cb = cur.reshape(h // 8, 8, bw, 8).transpose(0, 2, 1, 3).reshape(nb, 8, 8).astype(np.int16)
    satd = oracle.satd8x8((cb - pred).reshape(nb, 64), threads=8)
    assert np.array_equal(satd, best["cost"]), "%s: a winner's SATD differs from the oracle's" % what
    own = np.clip(seeds.astype(np.int64)[((by >> scale) * gw + (bx >> scale))] << scale, -R.CLAMP, R.CLAMP)
    table = np.array([R.code_length(d) for d in range(-512, 513)], np.int64)      # a neighbour's centre lies at most 2 * 64 + r from the own one
    d = np.stack([best["mvx"], best["mvy"]], axis=1).astype(np.int64) - own
    assert np.abs(d).max() <= 512
    assert np.array_equal(j, satd + ((lam * (table[d[:, 0] + 512] + table[d[:, 1] + 512])) >> 4)), "%s: d_j differs" % what
    say("%s: %d winners' SATD and J agree with the oracle and tests/_seeded_ref.py's vector cost" % (what, nb))
    return satd


def measure(codec, ev, w, h, say):
    import _seeded_ref as R
    from _util import Oracle, me_frames
    oracle = Oracle()
    n, nb = (w // 16) * (h // 16), (w // 8) * (h // 8)
    cur, ref = me_frames(w, h, 0, 0x2121, mv=(11, -7))
    al = codec.alloc
    d = dict(cur=al(n * 512), ref=al(n * 512), low=al(n * 128), ref_low=al(n * 128), low_best=al(8 * n), best=al(8 * nb), j=al(4 * nb), full=al(8 * nb),
             best0=al(8 * nb), j0=al(4 * nb))
    d["cur"].upload(R.tiles_of(oracle, cur, 1))
    d["ref"].upload(R.tiles_of(oracle, ref, 2))
    p_low = [codec.la_params(w, h, d_src=d[a].ptr, d_low=d[b].ptr) for a, b in (("cur", "low"), ("ref", "ref_low"))]
    seeded = lambda r, centres=31: codec.seed_params(w, h, 1, centres, r, 16, d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_seed=d["low_best"].ptr, d_best=d["best"].ptr,
                                                     d_j=d["j"].ptr)
    p_r = {r: seeded(r) for r in (0, 2, 8)}
    p_block = codec.seed_params(w, h, 0, 31, 2, 16, d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_seed=d["full"].ptr, d_best=d["best0"].ptr, d_j=d["j0"].ptr)
    low_search = lambda: codec.satd_search_from_tiles_dev(d["low"].ptr, d["ref_low"].ptr, w // 2, h // 2, 32, d["low_best"].ptr)
    full_search = lambda: codec.satd_search_from_tiles_dev(d["cur"].ptr, d["ref"].ptr, w, h, 64, d["full"].ptr)

    def hier():
        low_search()
        codec.satd_seeded_search_dev(p_r[2])

    # one pass, checked on the host
    for p in p_low:
        codec.la_downscale_dev(p)
    hier()
    full_search()
    codec.satd_seeded_search_dev(p_block)
    codec.stream_sync()
    low_best = d["low_best"].download(np.uint8, 8 * n).view(R.ME_DTYPE)
    seeds = np.stack([low_best["mvx"], low_best["mvy"]], axis=1)
    best, j = d["best"].download(np.uint8, 8 * nb).view(R.ME_DTYPE), d["j"].download(np.uint32, nb)
    full = d["full"].download(np.uint8, 8 * nb).view(R.ME_DTYPE)
    say("\n%d x %d: %d blocks, %d seed cells; me_frames pair moved by (11, -7)" % (w, h, nb, n))
    satd = check(oracle, cur, ref, seeds, 1, 16, best, j, say, "(a) seed_scale 1, centres 31, r 2")
    same = (best["mvx"] == full["mvx"]) & (best["mvy"] == full["mvy"])
    say("(a) against (b): the same vector in %.1f %% of the blocks, (11, -7) in %.1f %% of (a)'s and %.1f %% of (b)'s; sum of SATD %d against %d (%.3f)"
        % (100.0 * same.mean(), 100.0 * ((best["mvx"] == 11) & (best["mvy"] == -7)).mean(), 100.0 * ((full["mvx"] == 11) & (full["mvy"] == -7)).mean(),
           int(satd.sum()), int(full["cost"].sum()), satd.sum() / max(int(full["cost"].sum()), 1)))
    check(oracle, cur, ref, np.stack([full["mvx"], full["mvy"]], axis=1), 0, 16, d["best0"].download(np.uint8, 8 * nb).view(R.ME_DTYPE),
          d["j0"].download(np.uint32, nb), say, "seed_scale 0 on (b)'s field, centres 31, r 2")

    calls = {"(a) lowres + seeded": hier, "(b) exhaustive +-64": full_search, "lowres search +-32": low_search,
             "seeded r = 0": lambda: codec.satd_seeded_search_dev(p_r[0]), "seeded r = 2": lambda: codec.satd_seeded_search_dev(p_r[2]),
             "seeded r = 8": lambda: codec.satd_seeded_search_dev(p_r[8]), "seeded, per block r = 2": lambda: codec.satd_seeded_search_dev(p_block),
             "downscale x 2": lambda: [codec.la_downscale_dev(p) for p in p_low]}
    cands = lambda r: 6 * (2 * r + 1) ** 2
    satds = {"(a) lowres + seeded": n * 65 * 65 + nb * cands(2), "(b) exhaustive +-64": nb * 129 * 129, "lowres search +-32": n * 65 * 65, "seeded r = 0": nb * cands(0),
             "seeded r = 2": nb * cands(2), "seeded r = 8": nb * cands(8), "seeded, per block r = 2": nb * cands(2), "downscale x 2": 0}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in calls.values():                                           # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d back-to-back calls, all legs alternating; SATDs: candidates scored (interior cells: six centres)" % (ROUNDS, REPS))
    say("%-26s %9s %9s %9s %12s %10s" % ("leg", "us", "min us", "max us", "SATDs", "GSATD/s"))
    for k in calls:
        say("%-26s %9.1f %9.1f %9.1f %12d %10.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, satds[k], satds[k] / t[k] / 1e6))
    a, b = t["(a) lowres + seeded"], t["(b) exhaustive +-64"]
    say("(a) / (b) = %.3f: the hierarchy takes %s time than the exhaustive search (%.1f x), scoring %.1f x fewer SATDs"
        % (a / b, "LESS" if a < b else "MORE", b / a, satds["(b) exhaustive +-64"] / satds["(a) lowres + seeded"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r21_seeded_search.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    measure(codec, ev, 3840, 2176, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
