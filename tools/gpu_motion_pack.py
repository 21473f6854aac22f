#!/usr/bin/env python3
"""Timing of the compact motion stream (xMotionPackGpu, xMotionUnpackGpu) at 3840 x 2176 (4K padded to whole CTUs) on the decided field of
tools/gpu_partition.py (its frames, lowres + seeded search + refinement, xInterPartitionDecideGpu at range 1, lambda_q4 64), all in ONE
process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  device legs (device events)   pack count-only; pack with a stream of exactly the total; unpack; and the box's read stream
                                (xHipMemCeilingDev, kind 1) over the 8 + 1 bytes per block of d_out and d_level, the bytes pack may read
  host legs (host clock, from   dense: what a host does today, the device-to-host copies of d_out and d_level;
  a synchronised device to      compact: the copies of the records and then of the stream's written words (their number from the last record);
  the last byte on the host)    pack + compact: the pack call, its sync and those copies -- the whole way of the new path

The host buffers are allocated once, so no leg pays for fresh pages.  The records and the stream are checked against tests/_motion_ref.py
before anything is timed, the unpacked field against d_out and d_level, and `bits` is printed beside the decision's own d_ctu.bits (the same
accounting under the other predictor).  No rate is a pass / fail condition; nothing is claimed about bitrate.
Usage: gpu_motion_pack.py [--out FILE] [--size W H]   (default profiles/r28_motion_pack.txt, 3840 2176)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.motion as X  # noqa: E402
import x266_amd.partition as P  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402

ROUNDS, REPS = 12, 20
LAMBDA = 64


def decided_field(codec, w, h):
    """d_out, d_level and d_ctu of the partition decision on gpu_partition.py's pair"""
    import _seeded_ref as S
    from _util import Oracle, me_frames
    oracle = Oracle()
    n, nb, n_ctu = (w // 16) * (h // 16), (w // 8) * (h // 8), ((w + 63) // 64) * ((h + 63) // 64)
    cur, ref = me_frames(w, h, 0, 0x2121, mv=(11, -7))
    al = codec.alloc
    d = dict(cur=al(n * 512), ref=al(n * 512), low=al(n * 128), ref_low=al(n * 128), low_best=al(8 * n), best=al(8 * nb), q=al(8 * nb), out=al(8 * nb), level=al(nb),
             ctu=al(16 * n_ctu))
    d["cur"].upload(S.tiles_of(oracle, cur, 1))
    d["ref"].upload(S.tiles_of(oracle, ref, 2))
    for a, b in (("cur", "low"), ("ref", "ref_low")):
        codec.la_downscale_dev(codec.la_params(w, h, d_src=d[a].ptr, d_low=d[b].ptr))
    codec.satd_search_from_tiles_dev(d["low"].ptr, d["ref_low"].ptr, w // 2, h // 2, 32, d["low_best"].ptr)
    codec.satd_seeded_search_dev(codec.seed_params(w, h, 1, 31, 2, 16, d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_seed=d["low_best"].ptr, d_best=d["best"].ptr))
    codec.satd_refine_qpel_from_tiles_dev(d["cur"].ptr, d["ref"].ptr, w, h, d["best"].ptr, d["q"].ptr)
    codec.inter_partition_decide_dev(P.part_params(d_cur=d["cur"].ptr, d_ref=d["ref"].ptr, d_mv=d["q"].ptr, d_out=d["out"].ptr, d_level=d["level"].ptr, d_ctu=d["ctu"].ptr,
                                                   width=w, height=h, range=1, lambda_q4=LAMBDA))
    codec.stream_sync()
    return d["out"], d["level"], d["ctu"]


def measure(codec, ev, w, h, say):
    import _motion_ref as M
    nb, n_ctu = (w // 8) * (h // 8), ((w + 63) // 64) * ((h + 63) // 64)
    d_out, d_level, d_part = decided_field(codec, w, h)
    out = d_out.download(np.uint8, 8 * nb).view(M.ME_DTYPE)
    level = d_level.download(np.uint8, nb)
    part = d_part.download(np.uint8, 16 * n_ctu).view(x266_amd.PART_CTU_DTYPE)
    d_ctu, d_total, d_mv2, d_level2 = codec.alloc(32 * n_ctu), codec.alloc(16), codec.alloc(8 * nb), codec.alloc(nb)
    count = X.motion_params(d_mv=d_out.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_total=d_total.ptr, width=w, height=h)
    codec.motion_pack_dev(count)
    codec.stream_sync()
    words = int(d_total.download(np.uint64, 2)[0])
    d_stream = codec.alloc(2 * words)
    full = X.motion_params(d_mv=d_out.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr, d_total=d_total.ptr, width=w, height=h, cap_words=words)
    back = X.motion_params(d_mv=d_mv2.ptr, d_level=d_level2.ptr, d_ctu=d_ctu.ptr, d_stream=d_stream.ptr, width=w, height=h, cap_words=words)

    # one pass, checked against the reference and against the dense field
    codec.motion_pack_dev(full)
    codec.motion_unpack_dev(back)
    codec.stream_sync()
    ctu, stream, total = d_ctu.download(np.uint8, 32 * n_ctu).view(M.CTU_DTYPE), d_stream.download(np.uint16, words), d_total.download(np.uint64, 2)
    r = M.pack(np.stack([out["mvx"], out["mvy"]], axis=1), level, w, h)
    assert np.array_equal(ctu, r["ctu"]) and np.array_equal(stream, r["stream"]) and total.tolist() == r["total"].tolist(), "pack differs from the reference"
    mv2, level2 = d_mv2.download(np.uint8, 8 * nb).view(M.ME_DTYPE), d_level2.download(np.uint8, nb)
    assert np.array_equal(mv2["mvx"], out["mvx"]) and np.array_equal(mv2["mvy"], out["mvy"]) and not mv2["cost"].any() and np.array_equal(level2, level)
    parts = int(ctu["parts"].sum())
    assert parts == int(part["parts"].sum())
    dense_bytes, compact_bytes = 9 * nb, 32 * n_ctu + 2 * words
    say("\n%d x %d: %d blocks, %d CTUs; the decided field of lowres + seeded search + refinement + xInterPartitionDecideGpu (range 1, lambda_q4 %d)" % (w, h, nb, n_ctu, LAMBDA))
    say("partitions per level %s, %d in all; records, stream and totals equal tests/_motion_ref.py's, unpack returns d_out's vectors and d_level"
        % ([int(np.bincount(level, minlength=4)[k]) >> (2 * k) for k in range(4)], parts))
    say("bytes: dense d_out + d_level %d; compact %d = %d (records) + %d (stream, %d words): %.3f of the dense" %
        (dense_bytes, compact_bytes, 32 * n_ctu, 2 * words, words, compact_bytes / dense_bytes))
    say("bits (flags + Exp-Golomb of the differences to the causal predictor) %d, largest |difference| %d; d_ctu.bits of the decision (the same accounting, its "
        "own predictor from the input field) %d: ratio %.3f" % (int(ctu["bits"].sum()), int(ctu["max_abs"].max()), int(part["bits"].sum()),
                                                              int(ctu["bits"].sum()) / max(1, int(part["bits"].sum()))))

    # ---- device legs
    read_bytes = (8 * nb) // 16 * 16, nb // 16 * 16
    sums = codec.alloc(8 * nb // 2048 * 4 + 64)
    calls = {"pack, count-only": lambda: codec.motion_pack_dev(count), "pack": lambda: codec.motion_pack_dev(full), "unpack": lambda: codec.motion_unpack_dev(back),
             "read d_out + d_level": lambda: (codec.mem_ceiling_dev(1, d_out.ptr, sums.ptr, read_bytes[0]), codec.mem_ceiling_dev(1, d_level.ptr, sums.ptr, read_bytes[1]))}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    # ---- host legs: buffers allocated and touched once
    host = dict(out=np.ones(8 * nb, np.uint8), level=np.ones(nb, np.uint8), ctu=np.ones(32 * n_ctu, np.uint8), stream=np.ones(words, np.uint16))

    def copy(name, src, nbytes):
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, host[name].ctypes.data, src.ptr, nbytes), "xHipMemcpyD2H")

    def dense():
        copy("out", d_out, 8 * nb)
        copy("level", d_level, nb)

    def compact():
        copy("ctu", d_ctu, 32 * n_ctu)
        last = host["ctu"].view(M.CTU_DTYPE)[-1]                            # the stream ends where the last record's payload ends: no copy of d_total
        copy("stream", d_stream, 2 * (int(last["offset"]) + int(last["n_words"])))

    def pack_and_compact():
        codec.motion_pack_dev(full)
        codec.stream_sync()
        compact()

    hosts = {"host: dense copy": dense, "host: compact copy": compact, "host: pack + compact copy": pack_and_compact}

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
    assert np.array_equal(host["ctu"].view(M.CTU_DTYPE), r["ctu"]) and np.array_equal(host["stream"], r["stream"]) and np.array_equal(host["out"].view(M.ME_DTYPE), out)
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d back-to-back repetitions, all legs alternating; device legs by device events, host legs by the host's clock" % (ROUNDS, REPS))
    say("%-28s %10s %10s %10s" % ("leg", "us", "min us", "max us"))
    for k in ms:
        say("%-28s %10.1f %10.1f %10.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3))
    say("pack / read stream of d_out + d_level = %.2f; count-only / pack = %.2f; unpack / pack = %.2f"
        % (t["pack"] / t["read d_out + d_level"], t["pack, count-only"] / t["pack"], t["unpack"] / t["pack"]))
    a, b, c = t["host: dense copy"], t["host: compact copy"], t["host: pack + compact copy"]
    say("compact copy / dense copy = %.3f; pack + compact copy / dense copy = %.3f: the new path takes %s time than the dense copy it replaces"
        % (b / a, c / a, "LESS" if c < a else "MORE"))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r28_motion_pack.txt")
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
