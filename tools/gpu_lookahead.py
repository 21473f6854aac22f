#!/usr/bin/env python3
"""Timing of the lookahead at 3840 x 2176 (4K padded to whole CTUs), device events after warm-up, all in ONE process, the legs alternating
within every round, 10 % trimmed mean over the rounds:

  downscale           xLaDownscaleGpu: the half-size frame, 4 x 384 bytes read and 384 written per lowres tile
  intra costs         xLaIntraCostsGpu on that frame, costs and modes
  frame cost          xLaFrameCostGpu with one list: the block records (one launch) and the totals (one workgroup), as a caller pays for them
  propagate           xLaPropagateGpu with the vectors of a real search of the lowres frame against a moved copy
  propagate, one      the same with every block pointing into one block: all atomic adds on four addresses, the most contention there is
  tree qp             xLaTreeQpGpu, both outputs, with AQ offsets
  read 384 / 512      this box's read stream (xHipMemCeilingDev X266_MEM_READ) over as many bytes as the downscale reads of the frame
                      (m_Y + m_C: 384 bytes per tile) and as the frame holds (512 per tile), in the same run

"of read" = read-stream time of 384 bytes per tile / downscale time.  No rate is a pass / fail condition.
The calls are short enough for the launch to show in an event timing, and xLaFrameCostGpu is two launches, so the kernels apart come from
a kernel trace of this same script, taken in a run of its own (the profiler slows the host):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_lookahead.py --launch-only
  python tools/gpu_lookahead.py --kernel-stats DIR

The source is a smooth field with edges, flat patches and noise; every result but the search's is checked against tests/_la_ref.py.
Usage: gpu_lookahead.py [--out FILE] [--kernel-stats DIR] [--launch-only]   (default profiles/r20_lookahead.txt)"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from gpu_aq import source, trimmed_mean  # noqa: E402

ROUNDS, REPS = 20, 20
KERNELS = ("la_downscale_kernel", "la_intra_costs_kernel", "la_frame_cost_kernel", "la_totals_kernel", "la_propagate_kernel", "la_tree_qp_kernel",
           "mem_ceiling_kernel")


def kernel_split(directory):
    """{kernel: [(calls, mean us), ...]} from the kernel statistics a trace of --launch-only left under `directory`"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    calls = int(float(row["Calls"]))
                    out.setdefault(k, []).append((calls, float(row["TotalDurationNs"]) / calls / 1e3, row["Name"][:60]))
    return out


def measure(codec, ev, w, h, say, launch_only):
    import _la_ref as R
    n, n_ctu = (w // 16) * (h // 16), codec.ctu_count(w, h)
    bw = w // 16
    tiles = source(w, h)
    moved_tiles = R.shifted(tiles, w, h, 6, -4)
    al = codec.alloc
    d = dict(src=al(n * 512), ref=al(n * 512), low=al(n * 128), ref_low=al(n * 128), intra=al(4 * n), mode=al(n), best=al(8 * n), one=al(8 * n), block=al(16 * n),
             block_one=al(16 * n), total=al(64), prop=al(8 * n), acc=al(8 * n), aq=al(2 * n), off=al(2 * n), qp=al(6 * n_ctu))
    d["src"].upload(tiles)
    d["ref"].upload(moved_tiles)
    zeros = np.zeros(n, np.uint64)
    prop = np.random.RandomState(20).randint(0, 1 << 20, n).astype(np.uint64)
    aq = np.random.RandomState(21).randint(-768, 769, n).astype(np.int16)
    d["prop"].upload(prop)
    d["aq"].upload(aq)
    d["acc"].upload(zeros)
    common = dict(d_low=d["low"].ptr, d_intra=d["intra"].ptr, d_mode=d["mode"].ptr, d_total=d["total"].ptr, d_prop=d["prop"].ptr, d_prop_ref0=d["acc"].ptr,
                  d_aq_offset=d["aq"].ptr, d_offset=d["off"].ptr, d_qp=d["qp"].ptr)
    p = codec.la_params(w, h, 64, 512, 32, 0, d_src=d["src"].ptr, d_inter0=d["best"].ptr, d_block=d["block"].ptr, **common)
    p_ref = codec.la_params(w, h, d_src=d["ref"].ptr, d_low=d["ref_low"].ptr)
    p_one = codec.la_params(w, h, 64, 512, 32, 0, d_src=d["src"].ptr, d_inter0=d["one"].ptr, d_block=d["block_one"].ptr, **common)

    # one pass, checked against the restatement
    codec.la_downscale_dev(p)
    codec.la_downscale_dev(p_ref)
    codec.la_intra_costs_dev(p)
    codec.satd_search_from_tiles_dev(d["low"].ptr, d["ref_low"].ptr, w // 2, h // 2, 8, d["best"].ptr)
    codec.stream_sync()
    best = d["best"].download(np.uint8, 8 * n).view(R.ME_DTYPE)
    one = best.copy()                                                       # every block points into block (bw / 2, 3), a little off the grid
    one["mvx"], one["mvy"] = 8 * (bw // 2 - np.arange(n) % bw) + 3, 8 * (3 - np.arange(n) // bw) + 5
    d["one"].upload(one.view(np.uint8))
    codec.la_frame_cost_dev(p_one)
    codec.la_frame_cost_dev(p)
    codec.la_propagate_dev(p)
    codec.la_tree_qp_dev(p)
    codec.stream_sync()
    low = R.downscale(tiles, w, h)
    assert np.array_equal(d["low"].download(np.uint8, n * 128).reshape(-1, 512)[:, :384], low[:, :384]), "the lowres frame differs from tests/_la_ref.py"
    cost, mode = R.intra_costs(low, w, h)
    assert np.array_equal(d["intra"].download(np.uint32, n), cost) and np.array_equal(d["mode"].download(np.uint8, n), mode), "the intra costs differ"
    rec, tot = R.frame_cost(cost, mode, best, None, 64)
    assert np.array_equal(d["block"].download(np.uint8, 16 * n).view(R.BLOCK_DTYPE), rec) and d["total"].download(np.int64, 8).tolist() == tot.tolist(), "the records differ"
    acc, _ = R.propagate(rec, prop, zeros, None, w, h)
    assert np.array_equal(d["acc"].download(np.uint64, n), acc), "the accumulator differs"
    want_off, want_qp = R.tree_qp(rec, prop, aq, w, h, 512, 32, 0)
    got_qp = d["qp"].download(np.uint8, 6 * n_ctu)
    assert np.array_equal(d["off"].download(np.int16, n), want_off) and np.array_equal(got_qp, want_qp), "the qp map differs"
    say("\n%d x %d (%d blocks, %d CTUs): intra cost %d..%d, modes %s; P decision: %d intra, %d list 0, cost %d against intra %d; handed on %d in all, "
        "at most %d to one block; qp map at base 32, strength 2.0: %d..%d"
        % (w, h, n, n_ctu, int(cost.min()), int(cost.max()), dict(zip(*[a.tolist() for a in np.unique(mode, return_counts=True)])), tot[2], tot[3], tot[0],
           tot[1], int(acc.sum()), int(acc.max()), int(got_qp.min()), int(got_qp.max())))

    sums = al(n * 512 // 2048 * 4 + 16)
    calls = {"downscale": lambda: codec.la_downscale_dev(p), "intra costs": lambda: codec.la_intra_costs_dev(p), "frame cost": lambda: codec.la_frame_cost_dev(p),
             "propagate": lambda: codec.la_propagate_dev(p), "propagate, one": lambda: codec.la_propagate_dev(p_one), "tree qp": lambda: codec.la_tree_qp_dev(p),
             "read 384 B / tile": lambda: codec.mem_ceiling_dev(1, d["src"].ptr, sums.ptr, n * 384),
             "read 512 B / tile": lambda: codec.mem_ceiling_dev(1, d["src"].ptr, sums.ptr, n * 512)}
    moved = {"downscale": n * 384 + n // 4 * 384, "intra costs": n // 4 * 256 + 5 * n, "frame cost": 13 * n + 2 * 16 * n + 8 * n + 64,
             "propagate": 24 * n + 4 * 8 * n, "propagate, one": 24 * n + 4 * 8 * n, "tree qp": 16 * n + 8 * n + 4 * n + 6 * n_ctu,
             "read 384 B / tile": n * 384, "read 512 B / tile": n * 512}

    if launch_only:                                                     # the contended step apart: its kernel's mean would hide the spread one
        for k in calls:
            if k != "propagate, one":
                for _ in range(200):
                    calls[k]()
        codec.stream_sync()
        return

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
    say("10 %% trimmed mean of %d rounds of %d back-to-back calls, all legs alternating; GB/s over the bytes a leg reads and writes" % (ROUNDS, REPS))
    say("%-22s %9s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "GB/s", "of read"))
    for k in calls:
        of = "%9.3f" % (t["read 384 B / tile"] / t[k]) if k == "downscale" else ""
        say("%-22s %9.2f %9.2f %9.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, moved[k] / t[k] / 1e6, of))
    say("propagate, all blocks into one / spread by a search: %.2f" % (t["propagate, one"] / t["propagate"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r20_lookahead.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    if "--launch-only" in argv:
        measure(codec, ev, 3840, 2176, lambda s="": None, True)
        return
    say("device: %s" % (codec.device_info(),))
    measure(codec, ev, 3840, 2176, say, False)
    for e in ev:
        codec.event_destroy(e)
    if "--kernel-stats" in argv:
        split = kernel_split(argv[argv.index("--kernel-stats") + 1])
        say("\nthe kernels apart, from rocprofv3 --kernel-trace --stats over `gpu_lookahead.py --launch-only` (a run of its own; the propagate step")
        say("there is the one spread by a search; the read stream's rows are 384 and 512 bytes per tile together):")
        say("%-24s %9s %9s" % ("kernel", "calls", "mean us"))
        for k in KERNELS:
            for calls, mean, name in split.get(k, []):
                say("%-24s %9d %9.2f   %s" % (k, calls, mean, name))
            if k not in split:
                say("%-24s not measured (no row for it in the trace)" % k)
    else:
        say("\nthe kernels apart: not measured in this run (see --kernel-stats)")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
