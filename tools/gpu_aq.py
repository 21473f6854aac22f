#!/usr/bin/env python3
"""Timing of the source analysis at 3840 x 2176 (4K padded to whole CTUs), device events after warm-up, all in ONE process, the legs
alternating within every round, 10 % trimmed mean over the rounds:

  stats + totals      xAqStatsGpu: the tile records (one launch over the frame) and the totals (one workgroup), as a caller pays for them
  decide              xAqDecideGpu, mode 2, both outputs
  read 384 / 512      this box's read stream (xHipMemCeilingDev X266_MEM_READ) over as many bytes as the statistics use of the frame
                      (m_Y + m_C: 384 bytes per tile) and as the frame holds (512 per tile), in the same run

"of read" = read-stream time of 384 bytes per tile / call time.  No rate is a pass / fail condition.
The three kernels apart: the two launches of xAqStatsGpu have no entry point of their own, so their split comes from a kernel trace of
this same script, taken in a run of its own (the profiler slows the host):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_aq.py --launch-only
  python tools/gpu_aq.py --kernel-stats DIR

The source is a smooth field with edges, flat patches and Gaussian noise, so that tiles of every activity occur; the tool reports the
spread of the qp map the decision makes of it and checks records, totals and map against tests/_aq_ref.py.
Usage: gpu_aq.py [--out FILE] [--kernel-stats DIR] [--launch-only]   (default profiles/r19_aq.txt)"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS = 20, 20
KERNELS = ("aq_stats_kernel", "aq_totals_kernel", "aq_decide_kernel")


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def plane(rs, pw, ph, scale):
    yy, xx = np.mgrid[0:ph, 0:pw] * scale
    field = 40 * np.sin(xx / 7.0) * np.cos(yy / 11.0) + 25 * np.sin((xx + 2 * yy) / 17.0)
    edges = 22 * np.sign(np.sin((xx + yy) / 9.0))
    busy = (np.sin(xx / 301.0) * np.cos(yy / 197.0)) > 0.2                 # patches of detail in a calm frame
    p = 128 + 30 * np.sin(xx / 900.0) + busy * (field + edges + rs.normal(0.0, 8.0, (ph, pw)))
    return np.clip(np.round(p), 0, 255).astype(np.uint8)


def source(w, h):
    import _aq_ref as R
    rs = np.random.RandomState(0x266)
    return R.tiles_from_planes(plane(rs, w, h, 1), plane(rs, w // 2, h // 2, 2), plane(rs, w // 2, h // 2, 2), 7)


def kernel_split(directory):
    """{kernel: (calls, mean us)} from the kernel statistics a trace of --launch-only left under `directory`"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    calls = int(float(row["Calls"]))
                    out[k] = (calls, float(row["TotalDurationNs"]) / calls / 1e3)
    return out


def measure(codec, ev, w, h, say, launch_only):
    import _aq_ref as R
    nt, n = (w // 16) * (h // 16), codec.ctu_count(w, h)
    tiles = source(w, h)
    src, tile, total, off, qp = codec.alloc(nt * 512), codec.alloc(nt * 32), codec.alloc(64), codec.alloc(nt * 2), codec.alloc(n * 6)
    src.upload(tiles)
    p = codec.aq_params(src.ptr, tile.ptr, total.ptr, off.ptr, qp.ptr, w, h, 2, 256, 32, 0)
    calls = {"stats + totals": lambda: codec.aq_stats_dev(p), "decide": lambda: codec.aq_decide_dev(p)}
    if launch_only:
        for _ in range(200):
            for fn in calls.values():
                fn()
        codec.stream_sync()
        return
    codec.aq_stats_dev(p)
    codec.aq_decide_dev(p)
    codec.stream_sync()
    rec, tot = tile.download(np.uint8, nt * 32).view(R.TILE_DTYPE), total.download(np.int64, 8)
    want = R.tile_stats(tiles)
    assert np.array_equal(rec, want) and tot.tolist() == R.totals(want).tolist(), "the records differ from tests/_aq_ref.py"
    want_off, want_qp = R.decide(want, tot, w, h, 2, 256, 32, 0)
    got_qp = qp.download(np.uint8, n * 6)
    assert np.array_equal(off.download(np.int16, nt), want_off) and np.array_equal(got_qp, want_qp), "the qp map differs from tests/_aq_ref.py"
    say("\n%d x %d (%d tiles, %d CTUs): log2_q8 %d..%d, frame mean %d; qp map at base 32, strength 1.0, mode 2: %d..%d, bytes per value %s"
        % (w, h, nt, n, int(rec["log2_q8"].min()), int(rec["log2_q8"].max()), int((tot[6] + nt // 2) // nt), int(got_qp.min()), int(got_qp.max()),
           dict(zip(*[a.tolist() for a in np.unique(got_qp, return_counts=True)]))))

    moved = {"stats + totals": nt * 384 + 2 * nt * 32 + 64, "decide": nt * 6 + 64 + nt * 2 + n * 6, "read 384 B / tile": nt * 384, "read 512 B / tile": nt * 512}
    sums = codec.alloc(nt * 512 // 2048 * 4 + 16)
    calls["read 384 B / tile"] = lambda: codec.mem_ceiling_dev(1, src.ptr, sums.ptr, nt * 384)
    calls["read 512 B / tile"] = lambda: codec.mem_ceiling_dev(1, src.ptr, sums.ptr, nt * 512)

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
        of = "" if k.startswith("read") else "%9.3f" % (t["read 384 B / tile"] / t[k])
        say("%-22s %9.2f %9.2f %9.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, moved[k] / t[k] / 1e6, of))
    return t, nt


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r19_aq.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    if "--launch-only" in argv:
        measure(codec, ev, 3840, 2176, say, True)
        return
    say("device: %s" % (codec.device_info(),))
    t, nt = measure(codec, ev, 3840, 2176, say, False)
    for e in ev:
        codec.event_destroy(e)
    if "--kernel-stats" in argv:
        split = kernel_split(argv[argv.index("--kernel-stats") + 1])
        say("\nthe kernels apart, from rocprofv3 --kernel-trace --stats over `gpu_aq.py --launch-only` (a run of its own):")
        say("%-22s %9s %9s %9s" % ("kernel", "calls", "mean us", "of read"))
        for k in KERNELS:
            if k in split:
                of = "%9.3f" % (t["read 384 B / tile"] * 1e3 / split[k][1]) if k == "aq_stats_kernel" else ""
                say("%-22s %9d %9.2f %9s" % (k, split[k][0], split[k][1], of))
            else:
                say("%-22s not measured (no row for it in the trace)" % k)
    else:
        say("\nthe kernels apart: not measured in this run (see --kernel-stats)")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
