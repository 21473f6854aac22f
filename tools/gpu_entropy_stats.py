#!/usr/bin/env python3
"""Timing and byte counts of the per-context bin statistics (xEntropyStatsLevelsGpu, xEntropyStatsSideGpu, xEntropyInitFromCounts) at
3840 x 2176, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds.

Three frames, all 12 240 regions of 32x32:
  A   the coded frame of tools/gpu_entropy_side.py (profiles/r31_entropy_side.txt): kinds, modes, qp map, coded flags and levels of
      xDct32CodeMixedFrameGpu -- the frame whose side stream the host-found table took from 4 214 to 2 144 bytes
  B   the frame of tools/gpu_entropy.py (profiles/r29_entropy.txt) under the plain quantiser
  C   the same under RDOQ

  checks        d_counts of every frame against the sum of xEntropyCountRegion / xEntropyCountSideCtu over the frame on the host, the rows
                of d_part against the same per row, the sum against the ctx_bins of the count-only encode; the side table against the float
                rule of tools/gpu_entropy_side.py (best_static_table)
  device legs   (device events) the level statistics beside xLevelsBitsGpu, the count-only xEntropyEncodeLevelsGpu and the read stream of
                the touched level bytes; the side statistics beside the count-only xEntropyEncodeSideGpu
  bytes         level bytes of each frame under the default table, under its own table and under another frame's (A under B's, B under
                C's, C under B's: "the previous frame's table" between frames that differ far more than neighbours in a sequence do);
                side bytes of A under the default and under its own table

One figure is a condition: the level statistics must take less time than the count-only encode they stand in for; the tool fails
otherwise.  Nothing is claimed about bitrate beyond these bytes and no default table changes.
Usage: gpu_entropy_stats.py [--out FILE] [--size W H]   (default profiles/r32_entropy_stats.txt, 3840 2176)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.entropy as XE  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402
from gpu_entropy import LAMBDA, ROUNDING  # noqa: E402
from gpu_entropy_side import OFF, QP, best_static_table, coded_frame  # noqa: E402
from gpu_levels import frame_pair  # noqa: E402

ROUNDS, REPS = 12, 10
RR, CC = x266_amd.ENTROPY_STATS_REGIONS, x266_amd.ENTROPY_SIDE_STATS_CTUS


def host_level_counts(levels, nnz):
    """(the sum of xEntropyCountRegion over the frame, the same per row of RR regions)"""
    L = x266_amd.load_library()
    n = len(levels)
    part = np.zeros((XE.entropy_stats_rows(n, RR), 100, 2), np.uint64)
    for r in range(n):
        assert L.xEntropyCountRegion(levels[r].ctypes.data, 3, int(nnz[r] != 0), part[r // RR].ctypes.data) == 0
    return part.sum(axis=0), part


def host_side_counts(n_ctu, kind, mode, qps, nnz):
    part = np.zeros((XE.entropy_stats_rows(n_ctu, CC), 16, 2), np.uint64)
    for c in range(n_ctu):
        s = slice(6 * c, 6 * c + 6)
        XE.entropy_count_side_ctu(kind[s], mode[s], None, qps[s], nnz[s], QP, OFF, counts=part[c // CC])
    return part.sum(axis=0), part


def timed_legs(codec, ev, calls, say):
    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in calls.values():                                               # warm-up: code objects, clocks
        for _ in range(2):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("%-44s %10s %10s %10s" % ("leg", "us", "min us", "max us"))
    for k in ms:
        say("%-44s %10.1f %10.1f %10.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3))
    return t


def level_frame(codec, ev, name, d_level, d_nnz, n, say):
    """check and time one frame's level statistics -> (levels, nnz, counts, the frame's own table)"""
    al = codec.alloc
    levels, nnz = d_level.download(np.int16, n * 1024).reshape(n, 1024), d_nnz.download(np.uint32, n)
    rows = XE.entropy_stats_rows(n, RR)
    d_counts, d_part, d_region, d_total, d_stat = al(1600), al(800 * rows), al(32 * n), al(16), al(16 * n)
    p = XE.entropy_stats_params(d_level=d_level.ptr, d_nnz=d_nnz.ptr, d_counts=d_counts.ptr, d_part=d_part.ptr, n_regions=n)
    count = XE.entropy_params(d_level=d_level.ptr, d_nnz=d_nnz.ptr, d_region=d_region.ptr, d_total=d_total.ptr, n_regions=n)
    p_bits = codec.rdoq_params(0, d_level.ptr, 0, 0, d_nnz.ptr, d_stat.ptr, n)
    XE.entropy_stats_levels_dev(codec, p)
    codec.entropy_encode_levels_dev(count)
    codec.stream_sync()
    counts, part = d_counts.download(np.uint64, 200).reshape(100, 2), d_part.download(np.uint32, 200 * rows).reshape(rows, 100, 2)
    rec = d_region.download(np.uint8, 32 * n).view(x266_amd.ENTROPY_REGION_DTYPE)
    want, want_part = host_level_counts(levels, nnz)
    assert np.array_equal(counts, want) and np.array_equal(part, want_part), "the device's counts differ from the sum of xEntropyCountRegion"
    assert int(counts.sum()) == int(rec["ctx_bins"].astype(np.uint64).sum()), "the counts do not add up to the encoder's context bins"
    table = XE.entropy_init_from_counts(counts)
    say("\n%s: %d regions in %d rows, %d with a level; d_counts and every row of d_part equal the sum of xEntropyCountRegion; %d context bins = the count-only encode's"
        % (name, n, rows, int((nnz != 0).sum()), int(counts.sum())))
    say("size 32 counts zero/one: " + " ".join("%d/%d" % (z, o) for z, o in counts[75:]))
    say("its own table, size 32: " + " ".join(str(int(x)) for x in table[75:]) + "   (the default: 19 x 1024, then 1385 723 1242 1609 1325 1263)")
    touched = int((nnz != 0).sum()) * 2048
    sums = al(touched // 2048 * 4 + 64)
    t = timed_legs(codec, ev, {"xEntropyStatsLevelsGpu": lambda: XE.entropy_stats_levels_dev(codec, p),
                               "xLevelsBitsGpu": lambda: codec.levels_bits_dev(p_bits),
                               "xEntropyEncodeLevelsGpu, count-only": lambda: codec.entropy_encode_levels_dev(count),
                               "read stream, touched bytes": lambda: codec.mem_ceiling_dev(1, d_level.ptr, sums.ptr, touched)}, say)
    s, e, b, m = (t[k] for k in ("xEntropyStatsLevelsGpu", "xEntropyEncodeLevelsGpu, count-only", "xLevelsBitsGpu", "read stream, touched bytes"))
    say("statistics / count-only encode = %.4f (the condition: below 1); statistics / xLevelsBitsGpu = %.2f; statistics / read stream = %.2f; %.0f GB/s of touched bytes"
        % (s / e, s / b, s / m, touched / s / 1e6))
    assert s < e, "the level statistics (%.1f us) do not beat the count-only encode (%.1f us)" % (s * 1e3, e * 1e3)
    return levels, nnz, counts, table


def level_bytes(codec, levels, nnz, table):
    return int(XE.entropy_encode_levels(codec, levels, None, nnz, init=table)[0]["n_bytes"].sum())


def side_frame(codec, ev, n_ctu, kind, mode, qps, nnz, say):
    import _entropy_side_ref as S
    al = codec.alloc
    rows = XE.entropy_stats_rows(n_ctu, CC)
    arrays = dict(d_kind=kind, d_mode=mode, d_qp=qps, d_nnz=nnz)
    d_in = {name: codec._upload(np.ascontiguousarray(a)) for name, a in arrays.items()}
    ptrs = {name: d.ptr for name, d in d_in.items()}
    d_counts, d_part, d_coded, d_total = al(256), al(128 * rows), al(32 * n_ctu), al(16)
    p = XE.entropy_side_stats_params(d_counts=d_counts.ptr, d_part=d_part.ptr, n_ctu=n_ctu, qp=QP, chroma_qp_offset=OFF, **ptrs)
    enc0 = XE.entropy_side_params(d_coded=d_coded.ptr, d_total=d_total.ptr, n_ctu=n_ctu, qp=QP, chroma_qp_offset=OFF, **ptrs)
    XE.entropy_stats_side_dev(codec, p)
    XE.entropy_encode_side_dev(codec, enc0)
    codec.stream_sync()
    counts, part = d_counts.download(np.uint64, 32).reshape(16, 2), d_part.download(np.uint32, 32 * rows).reshape(rows, 16, 2)
    coded = d_coded.download(np.uint8, 32 * n_ctu).view(x266_amd.ENTROPY_SIDE_CTU_DTYPE)
    want, want_part = host_side_counts(n_ctu, kind, mode, qps, nnz)
    assert np.array_equal(counts, want) and np.array_equal(part, want_part), "the device's side counts differ from the sum of xEntropyCountSideCtu"
    assert int(counts.sum()) == int(coded["ctx_bins"].sum())
    table = XE.entropy_init_from_counts(counts)
    tool, zeros, ones = best_static_table(S, S.canon_arrays(n_ctu, kind, mode, None, qps, nnz, QP, OFF), QP, OFF)
    assert np.array_equal(zeros, counts[:, 0].astype(int)) and np.array_equal(ones, counts[:, 1].astype(int)), "the counts differ from the reference's bins"
    differ = [(c, int(table[c]), int(tool[c])) for c in range(16) if table[c] != tool[c]]
    default = int(coded["n_bytes"].sum())
    own = int(XE.entropy_encode_side(codec, n_ctu, kind, mode, None, qps, nnz, qp=QP, chroma_qp_offset=OFF, init=table)[0]["n_bytes"].sum())
    say("\nA, side information: %d CTUs in %d rows; d_counts and every row of d_part equal the sum of xEntropyCountSideCtu and the reference's bins; %d context bins"
        % (n_ctu, rows, int(counts.sum())))
    say("zero / one bins per context: " + " ".join("%d/%d" % (z, o) for z, o in counts))
    say("the table of xEntropyInitFromCounts: " + " ".join(str(int(x)) for x in table))
    say("against the float rule of tools/gpu_entropy_side.py: " + ("no entry differs" if not differ else "entries (context, integer, float) %s differ" % differ))
    say("side bytes under the default table %d, under the frame's own table from the device's counts %d (%.3f)" % (default, own, own / max(1, default)))
    t = timed_legs(codec, ev, {"xEntropyStatsSideGpu": lambda: XE.entropy_stats_side_dev(codec, p),
                               "xEntropyEncodeSideGpu, count-only": lambda: XE.entropy_encode_side_dev(codec, enc0)}, say)
    say("side statistics / count-only side encode = %.2f" % (t["xEntropyStatsSideGpu"] / t["xEntropyEncodeSideGpu, count-only"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r32_entropy_stats.txt")
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
    w, h = size
    n_ctu = codec.ctu_count(w, h)
    n = 6 * n_ctu
    say("%d x %d, qp %d; 10 %% trimmed mean of %d rounds of %d back-to-back repetitions, all legs of a table alternating; device events" % (w, h, QP, ROUNDS, REPS))
    kind, mode, qps, nnz_a, levels_a, _, _ = coded_frame(codec, w, h)
    d_a, d_nnz_a = codec._upload(np.ascontiguousarray(levels_a, np.int16)), codec._upload(np.ascontiguousarray(nnz_a, np.uint32))
    cur, pred = frame_pair(codec, w, h)
    coef, plain, rdoq, nnz_p, nnz_r = (codec.alloc(b) for b in (n * 2048, n * 2048, n * 2048, 4 * n, 4 * n))
    codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred.ptr, w, h, coef.ptr)
    codec.quant_regions_dev(0, coef.ptr, plain.ptr, n, 0, 0, QP, ROUNDING, nnz_p.ptr)
    codec.rdo_quant_dev(codec.rdoq_params(coef.ptr, rdoq.ptr, 0, 0, nnz_r.ptr, 0, n, QP, LAMBDA))
    codec.stream_sync()
    frames = {}
    for key, name, d_level, d_nnz in (("A", "A, the coded frame of profiles/r31_entropy_side.txt", d_a, d_nnz_a),
                                      ("B", "B, the frame of profiles/r29_entropy.txt, plain quantiser (rounding %d)" % ROUNDING, plain, nnz_p),
                                      ("C", "C, the same frame under RDOQ (lambda %d)" % LAMBDA, rdoq, nnz_r)):
        frames[key] = level_frame(codec, ev, name, d_level, d_nnz, n, say)
    say("\nlevel bytes of a frame under the default table, under its own table and under another frame's table")
    say("%-6s %12s %12s %8s %14s %8s" % ("frame", "default", "own", "ratio", "other's", "ratio"))
    for key, other in (("A", "B"), ("B", "C"), ("C", "B")):
        levels, nnz, _, table = frames[key]
        base, own, lent = level_bytes(codec, levels, nnz, None), level_bytes(codec, levels, nnz, table), level_bytes(codec, levels, nnz, frames[other][3])
        say("%-6s %12d %12d %8.4f %11d (%s) %8.4f" % (key, base, own, own / base, lent, other, lent / base))
    side_frame(codec, ev, n_ctu, kind, mode, qps, nnz_a, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
