#!/usr/bin/env python3
"""Timing and rate of the entropy coder of the level stream (xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu) at 3840 x 2176 (4K padded
to whole CTUs), qp 32, on two level sets of the same frame pair (tools/gpu_levels.py's): the plain quantiser's (rounding 171) and the RDOQ
chain's (lambda 368).  All in ONE process, the legs alternating within every round, median and spread over the rounds:

  device legs (device events)   encode count-only; encode with a stream of exactly the total; decode; and next to them on the same input
                                xLevelsPackGpu, xLevelsBitsGpu and the box's read stream (xHipMemCeilingDev, kind 1) over the bytes the calls
                                actually touch, 2 KiB per region with a non-zero count
  host legs (host clock)        the device-to-host copy of the coded words against that of the packed words; xEntropyEncodeRegion over the whole
                                frame on one CPU thread and on 16 (what a host would pay with the coder off the device)

Rate: the coded bits against the xLevelsBitsGpu total per frame, and the same ratio over the regions that hold a level (median, 5th and 95th
percentile).  The cost of the per-region context restart comes from tests/_entropy_ref.py on a SAMPLE of CTUs -- contexts carried across
a CTU's six regions against six restarts --, not from the frame.  Every record is checked against the host coder before anything is timed, a
sample of regions against the Python reference, and decode against the encoder's input.  No time and no rate is a pass / fail condition.  The
bits are the residual's alone: classes, modes, qp and motion are not coded.
Usage: gpu_entropy.py [--out FILE] [--size W H]   (default profiles/r29_entropy.txt, 3840 2176)"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.entropy as X  # noqa: E402
from gpu_levels import frame_pair  # noqa: E402

ROUNDS, REPS, QP, LAMBDA, ROUNDING = 12, 10, 32, 368, 171
SAMPLE_CTUS, SAMPLE_REGIONS, THREADS = 48, 96, 16


def host_coder(levels, threads):
    """xEntropyEncodeRegion over every region -> (seconds, n_bytes per region, bins per region)"""
    L = x266_amd.load_library()
    n = len(levels)
    n_bytes, bins, outs = np.zeros(n, np.int64), np.zeros((n, 2), np.uint32), [np.zeros(x266_amd.ENTROPY_MAX_BYTES, np.uint8) for _ in range(threads)]

    def work(t):
        for r in range(t, n, threads):
            n_bytes[r] = L.xEntropyEncodeRegion(levels[r].ctypes.data, 3, None, outs[t].ctypes.data, outs[t].size, bins[r].ctypes.data)

    t0 = time.perf_counter()
    if threads == 1:
        work(0)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, range(threads)))
    return time.perf_counter() - t0, n_bytes, bins


def measure(codec, ev, name, d_level, d_nnz, n, say):
    import _entropy_ref as E
    al = codec.alloc
    levels, nnz = d_level.download(np.int16, n * 1024).reshape(n, 1024), d_nnz.download(np.uint32, n)
    d_region, d_total, d_back, d_back_nnz, d_stat, d_lrec, d_ltotal = al(32 * n), al(16), al(2048 * n), al(4 * n), al(16 * n), al(32 * n), al(16)
    count = X.entropy_params(d_level=d_level.ptr, d_nnz=d_nnz.ptr, d_region=d_region.ptr, d_total=d_total.ptr, n_regions=n)
    codec.entropy_encode_levels_dev(count)
    lcount = codec.levels_params(d_level.ptr, 0, d_nnz.ptr, d_lrec.ptr, 0, d_ltotal.ptr, n, 0)
    codec.levels_pack_dev(lcount)
    codec.stream_sync()
    words, lwords = int(d_total.download(np.uint64, 2)[0]), int(d_ltotal.download(np.uint64, 2)[0])
    d_stream, d_lstream = al(2 * words), al(2 * lwords)
    full = X.entropy_params(d_level=d_level.ptr, d_nnz=d_nnz.ptr, d_region=d_region.ptr, d_stream=d_stream.ptr, d_total=d_total.ptr, n_regions=n, cap_words=words)
    back = X.entropy_params(d_level=d_back.ptr, d_nnz=d_back_nnz.ptr, d_region=d_region.ptr, d_stream=d_stream.ptr, n_regions=n, cap_words=words)
    lfull = codec.levels_params(d_level.ptr, 0, d_nnz.ptr, d_lrec.ptr, d_lstream.ptr, d_ltotal.ptr, n, lwords)
    p_bits = codec.rdoq_params(0, d_level.ptr, 0, 0, d_nnz.ptr, d_stat.ptr, n)

    # one pass, checked: decode against the input, every record against the host coder, a sample against the Python reference
    codec.entropy_encode_levels_dev(full)
    codec.entropy_decode_levels_dev(back)
    codec.levels_bits_dev(p_bits)
    codec.stream_sync()
    rec, stream = d_region.download(np.uint8, 32 * n).view(x266_amd.ENTROPY_REGION_DTYPE), d_stream.download(np.uint16, words)
    stat = d_stat.download(np.uint8, 16 * n).view(x266_amd.RDOQ_REGION_DTYPE)
    assert np.array_equal(d_back.download(np.int16, n * 1024).reshape(n, 1024), levels) and np.array_equal(d_back_nnz.download(np.uint32, n), nnz), "decode differs"
    host_s = {}
    host_s[1], host_bytes, host_bins = host_coder(levels, 1)
    assert np.array_equal(host_bytes, rec["n_bytes"]) and np.array_equal(host_bins[:, 0], rec["ctx_bins"]) and np.array_equal(host_bins[:, 1], rec["bypass_bins"])
    host_s[THREADS] = host_coder(levels, THREADS)[0]
    raw = stream.astype("<u2").tobytes()
    for r in np.linspace(0, n - 1, SAMPLE_REGIONS).astype(int):
        data = E.encode_region(levels[r], 3)[0]
        assert raw[2 * int(rec["offset"][r]):2 * int(rec["offset"][r]) + int(rec["n_bytes"][r])] == data, "region %d differs from the reference" % r
    coded_bits, est_bits = 8 * int(rec["n_bytes"].sum()), int(stat["bits"].sum()) / 16.0
    held = stat["bits"] > 0
    ratio = 8.0 * rec["n_bytes"][held] * 16.0 / stat["bits"][held]
    say("\n%s: %d regions, %d with a level, %d non-zero levels; records equal the host coder's, %d regions equal tests/_entropy_ref.py's, decode returns the input"
        % (name, n, int(held.sum()), int(nnz.sum()), SAMPLE_REGIONS))
    say("coded: %d bytes in %d words (the dense levels: %d bytes; the packed stream of xLevelsPackGpu: %d words); %d context bins, %d bypass bins"
        % (int(rec["n_bytes"].sum()), words, 2048 * n, lwords, int(rec["ctx_bins"].sum()), int(rec["bypass_bins"].sum())))
    say("rate: coded bits %d against the estimate of xLevelsBitsGpu %.0f: ratio %.4f per frame; per region with a level: median %.3f, 5th percentile %.3f, 95th %.3f"
        % (coded_bits, est_bits, coded_bits / est_bits, np.median(ratio), np.percentile(ratio, 5), np.percentile(ratio, 95)))
    # the context restart, on a sample of CTUs: six restarts against contexts carried across the CTU's six regions
    ctus = np.linspace(0, n // 6 - 1, SAMPLE_CTUS).astype(int)
    apart = together = 0
    for c in ctus:
        bins = [E.region_bins(levels[6 * c + q], 3) for q in range(6)]
        apart += sum(len(E.code_bins(b, E._init(None, 3))) for b in bins)
        together += len(E.code_bins([x for b in bins for x in b], E._init(None, 3)))
    say("context restart, a SAMPLE of %d CTUs (not the frame): six substreams %d bytes, one substream with contexts carried across the six regions %d bytes: "
        "the restart costs %.1f %% here (termination bytes included)" % (SAMPLE_CTUS, apart, together, 100.0 * (apart - together) / max(together, 1)))

    # ---- device legs
    touched = int((nnz != 0).sum()) * 2048
    sums = al(touched // 2048 * 4 + 64)
    calls = {"encode, count-only": lambda: codec.entropy_encode_levels_dev(count), "encode": lambda: codec.entropy_encode_levels_dev(full),
             "decode": lambda: codec.entropy_decode_levels_dev(back), "xLevelsPackGpu": lambda: codec.levels_pack_dev(lfull),
             "xLevelsBitsGpu": lambda: codec.levels_bits_dev(p_bits), "read stream, touched bytes": lambda: codec.mem_ceiling_dev(1, d_level.ptr, sums.ptr, touched)}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    host = dict(coded=np.ones(max(words, 1), np.uint16), packed=np.ones(max(lwords, 1), np.uint16))

    def copy(which, src, nbytes):
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, host[which].ctypes.data, src.ptr, nbytes), "xHipMemcpyD2H")

    hosts = {"host: copy of the coded words": lambda: copy("coded", d_stream, 2 * words), "host: copy of the packed words": lambda: copy("packed", d_lstream, 2 * lwords)}

    def host_timed(k):
        codec.stream_sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            hosts[k]()
        return (time.perf_counter() - t0) * 1e3 / REPS

    for fn in list(calls.values()) + list(hosts.values()):               # warm-up: code objects, clocks, the copy paths
        for _ in range(2):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in list(calls) + list(hosts)}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
        for k in hosts:
            ms[k].append(host_timed(k))
    say("median of %d rounds of %d back-to-back repetitions, all legs alternating; device legs by device events, host legs by the host's clock" % (ROUNDS, REPS))
    say("%-32s %10s %10s %10s" % ("leg", "median us", "min us", "max us"))
    for k in ms:
        say("%-32s %10.1f %10.1f %10.1f" % (k, np.median(ms[k]) * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    say("encode / xLevelsPackGpu = %.1f; encode / read stream = %.1f; count-only / encode = %.2f; decode / encode = %.2f"
        % (med["encode"] / med["xLevelsPackGpu"], med["encode"] / med["read stream, touched bytes"], med["encode, count-only"] / med["encode"], med["decode"] / med["encode"]))
    say("host coder (xEntropyEncodeRegion, one pass, the call loop in Python): %.1f ms on one thread, %.1f ms on %d: %.0f x and %.0f x the device's encode"
        % (host_s[1] * 1e3, host_s[THREADS] * 1e3, THREADS, host_s[1] * 1e3 / med["encode"], host_s[THREADS] * 1e3 / med["encode"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r29_entropy.txt")
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
    cur, pred = frame_pair(codec, w, h)
    n = 6 * codec.ctu_count(w, h)
    coef, plain, rdoq, nnz_p, nnz_r = (codec.alloc(b) for b in (n * 2048, n * 2048, n * 2048, 4 * n, 4 * n))
    codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred.ptr, w, h, coef.ptr)
    codec.quant_regions_dev(0, coef.ptr, plain.ptr, n, 0, 0, QP, ROUNDING, nnz_p.ptr)
    codec.rdo_quant_dev(codec.rdoq_params(coef.ptr, rdoq.ptr, 0, 0, nnz_r.ptr, 0, n, QP, LAMBDA))
    codec.stream_sync()
    say("%d x %d, qp %d: the me_frames pair through xDct32FwdCtuFromTilesDev; contexts restart per region, the table is the default and static per call" % (w, h, QP))
    measure(codec, ev, "plain quantiser (rounding %d)" % ROUNDING, plain, nnz_p, n, say)
    measure(codec, ev, "RDOQ (lambda %d)" % LAMBDA, rdoq, nnz_r, n, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
