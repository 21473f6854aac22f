#!/usr/bin/env python3
"""Timing of the compact level stream (xLevelsPackGpu, xLevelsUnpackGpu) at 3840 x 2176 on the levels xDct32CodeCtuTilesGpu emits at qp
22, 32 and 37, device events after warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the
rounds.  The frame pair is the me_frames generator of tests/_util.py (a smooth picture, its displaced and noisy copy as the
prediction), Y, U and V, packed into tiles on the device.

The pack call is three launches (count, scan, write) on one stream and the ABI has no call for a single one, so the legs are the
calls a host can make, and the steps follow by difference:

  count + scan             the count-only call (cap_words 0, d_stream NULL): records, offsets, totals
  count + scan + write     the full call into a stream of exactly the total
  scan (empty count)       the count-only call with a d_nnz of zeros: the count step reads no level, what remains is the records,
                           the one-workgroup scan and two launches
  unpack                   xLevelsUnpackGpu of that stream
  ", nnz"                  the same with d_nnz given (pack: regions with a zero count are not read; unpack: the counts are written)
  read of the dense bytes  this box's read stream (xHipMemCeilingDev X266_MEM_READ) over the 2 KiB-per-region levels
  D2H dense / D2H packed   xHipMemcpyD2H into pinned host memory of the dense levels, and of records + totals + stream; host clock
                           around the synchronous copies

"of read" = read-stream time / call time.  No rate is a pass / fail condition.
Usage: gpu_levels.py [--out FILE]   (default profiles/r18_levels.txt)"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from _util import me_frames  # noqa: E402

ROUNDS, REPS, ROUNDING = 20, 20, 171
QPS = (22, 32, 37)


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def frame_pair(codec, w, h):
    """(cur, pred) as device tile arrays"""
    out = []
    planes = [me_frames(w, h, 0, 0x901, mv=(3, -2), noise=6), me_frames(w // 2, h // 2, 0, 0x902, mv=(2, -1), noise=6),
              me_frames(w // 2, h // 2, 0, 0x903, mv=(2, -1), noise=6)]
    for f in range(2):
        d = [codec.alloc(p[f].size) for p in planes]
        for buf, p in zip(d, planes):
            buf.upload(np.ascontiguousarray(p[f][:p[f].shape[0], :p[f].shape[1]]))
        tiles = codec.alloc(w * h * 2)
        codec.conv_input_fmt_dev(tiles.ptr, d[0].ptr, d[1].ptr, d[2].ptr, w, w, h)
        codec.stream_sync()
        out.append(tiles)
    return out


def measure(codec, ev, w, h, qp, cur, pred, say):
    n = 6 * codec.ctu_count(w, h)
    dense = n * 2048
    level, level2, nnz, nnz2, zeros, recon = codec.alloc(dense), codec.alloc(dense), codec.alloc(4 * n), codec.alloc(4 * n), codec.alloc(4 * n), codec.alloc(w * h * 2)
    rec, tot, sums = codec.alloc(32 * n), codec.alloc(16), codec.alloc(4 * n)
    zeros.upload(np.zeros(n, np.uint32))
    codec.dct32_code_ctu_tiles_dev(cur.ptr, pred.ptr, w, h, 0, qp, ROUNDING, level.ptr, nnz.ptr, recon.ptr)
    count_only = codec.levels_params(level.ptr, 0, 0, rec.ptr, 0, tot.ptr, n, 0)
    codec.levels_pack_dev(count_only)
    codec.stream_sync()
    words = int(tot.download(np.uint64, 2)[0])
    stream = codec.alloc(max(2 * words, 16))
    full = codec.levels_params(level.ptr, 0, 0, rec.ptr, stream.ptr, tot.ptr, n, words)
    full_nnz = codec.levels_params(level.ptr, 0, nnz.ptr, rec.ptr, stream.ptr, tot.ptr, n, words)
    count_nnz = codec.levels_params(level.ptr, 0, nnz.ptr, rec.ptr, 0, tot.ptr, n, 0)
    empty = codec.levels_params(level.ptr, 0, zeros.ptr, rec.ptr, 0, tot.ptr, n, 0)
    back = codec.levels_params(level2.ptr, 0, 0, rec.ptr, stream.ptr, 0, n, words)
    back_nnz = codec.levels_params(level2.ptr, 0, nnz2.ptr, rec.ptr, stream.ptr, 0, n, words)
    codec.levels_pack_dev(full_nnz)
    codec.levels_unpack_dev(back_nnz)
    codec.stream_sync()
    counts = nnz.download(np.uint32, n)
    assert np.array_equal(level2.download(np.int16, n * 1024), level.download(np.int16, n * 1024)), "unpack(pack(x)) != x"
    assert np.array_equal(nnz2.download(np.uint32, n), counts) and tot.download(np.uint64, 2).tolist() == [words, n]
    records = rec.download(np.uint8, 32 * n).view(x266_amd.LEVEL_REGION_DTYPE)
    packed = 2 * words + 32 * n + 16
    say("\nqp %d: %d regions, %d of them all zero, %d coded CGs of %d, %d non-zero levels; dense %d bytes, packed %d bytes (stream %d + records %d + totals 16): "
        "dense / packed %.1f" % (qp, n, int((counts == 0).sum()), sum(bin(int(m)).count("1") for m in records["cg_mask"]), 64 * n, int(counts.sum()), dense, packed,
                                 2 * words, 32 * n, dense / packed))

    calls = {"count + scan": lambda: codec.levels_pack_dev(count_only), "count + scan, nnz": lambda: codec.levels_pack_dev(count_nnz),
             "count + scan + write": lambda: codec.levels_pack_dev(full), "count + scan + write, nnz": lambda: codec.levels_pack_dev(full_nnz),
             "scan (empty count)": lambda: codec.levels_pack_dev(empty),
             "unpack": lambda: codec.levels_unpack_dev(back), "unpack, nnz": lambda: codec.levels_unpack_dev(back_nnz),
             "read of the dense bytes": lambda: codec.mem_ceiling_dev(1, level.ptr, sums.ptr, dense)}

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
    say("10 %% trimmed mean of %d rounds of %d calls, all legs alternating" % (ROUNDS, REPS))
    say("%-28s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "of read"))
    for k in calls:
        say("%-28s %9.2f %9.2f %9.2f %9.3f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, t["read of the dense bytes"] / t[k]))
    say("by difference: count %.2f us, write %.2f us (with nnz: %.2f, %.2f); the scan's share of the full call %.2f" % (
        (t["count + scan"] - t["scan (empty count)"]) * 1e3, (t["count + scan + write"] - t["count + scan"]) * 1e3,
        (t["count + scan, nnz"] - t["scan (empty count)"]) * 1e3, (t["count + scan + write, nnz"] - t["count + scan, nnz"]) * 1e3,
        t["scan (empty count)"] / t["count + scan + write"]))

    # what crosses PCIe: the dense levels, or records + totals + stream, into pinned memory
    host = codec.host_alloc(dense, np.uint8)
    legs = {"D2H dense": [(level.ptr, dense)], "D2H packed": [(rec.ptr, 32 * n), (tot.ptr, 16), (stream.ptr, 2 * words)]}
    d2h = {k: [] for k in legs}
    for r in range(ROUNDS + 2):
        for k, parts in legs.items():
            codec.stream_sync()
            t0 = time.perf_counter()
            at = 0
            for ptr, nbytes in parts:
                if nbytes:
                    codec._check(codec.L.xHipMemcpyD2H(codec.ctx, ctypes.c_void_p(host.ctypes.data + at), ptr, nbytes), "xHipMemcpyD2H")
                at += (nbytes + 63) & ~63
            if r >= 2:                                                  # two warm-up rounds
                d2h[k].append(time.perf_counter() - t0)
    for k in legs:
        say("%-28s %9.2f us (min %.2f, max %.2f), host clock around the synchronous copies" % (k, trimmed_mean(d2h[k]) * 1e6, min(d2h[k]) * 1e6, max(d2h[k]) * 1e6))
    say("D2H dense / (full pack with nnz + D2H packed) %.2f" % (trimmed_mean(d2h["D2H dense"]) / (t["count + scan + write, nnz"] * 1e-3 + trimmed_mean(d2h["D2H packed"]))))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r18_levels.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    w, h = 3840, 2176
    say("%d x %d, scan step %d regions" % (w, h, x266_amd.levels_scan_chunk()))
    cur, pred = frame_pair(codec, w, h)
    for qp in QPS:
        measure(codec, ev, w, h, qp, cur, pred, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
