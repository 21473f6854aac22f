#!/usr/bin/env python3
"""Timing and byte counts of the entropy coder of the motion stream (xEntropyEncodeMvGpu, xEntropyDecodeMvGpu) and of xMotionReconstructGpu
at 3840 x 2176 on the decided field of tools/gpu_motion_pack.py (profiles/r28_motion_pack.txt), all in ONE process, the legs alternating
within every round, 10 % trimmed mean over the rounds:

  bytes         the coded bytes against sum(bits) / 8 of the pack records and against the packed records + stream
  device legs   (device events) pack and unpack (the yardsticks); encode count-only; encode with a stream of exactly the total; decode;
                reconstruct -- one launch per wavefront step, so bound by launches, not by work
  host leg      (host clock, from a synchronised device to the last byte on the host) the copy of the coded records and then of the coded
                words (their number from the last record), beside the same copy of the packed records and stream
  restart cost  the frame coded as ONE chain by tests/_entropy_ref.code_bins (contexts carried from CTU to CTU, one termination) against
                the sum of the independent substreams

Everything is checked against tests/_entropy_motion_ref.py and against the dense field before anything is timed.  No figure is a pass /
fail condition; the coded bytes are the motion's alone.
Usage: gpu_entropy_motion.py [--out FILE] [--size W H]   (default profiles/r30_entropy_motion.txt, 3840 2176)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.entropy as XE  # noqa: E402
import x266_amd.motion as XM  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402
from gpu_motion_pack import LAMBDA, decided_field  # noqa: E402

ROUNDS, REPS = 12, 10


def measure(codec, ev, w, h, say):
    import _entropy_motion_ref as EM
    import _entropy_ref as ER
    import _motion_ref as M
    nb, n_ctu = (w // 8) * (h // 8), ((w + 63) // 64) * ((h + 63) // 64)
    cw, ch = (w + 63) // 64, (h + 63) // 64
    d_out, d_level, _ = decided_field(codec, w, h)
    out = d_out.download(np.uint8, 8 * nb).view(M.ME_DTYPE)
    level = d_level.download(np.uint8, nb)
    al = codec.alloc
    d_ctu, d_total, d_coded, d_ctu2, d_words2, d_status, d_mv2, d_level2 = (al(32 * n_ctu), al(16), al(32 * n_ctu), al(32 * n_ctu), al(512 * n_ctu), al(max(n_ctu, 16)),
                                                                           al(8 * nb), al(nb))
    count = XM.motion_params(d_mv=d_out.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_total=d_total.ptr, width=w, height=h)
    codec.motion_pack_dev(count)
    codec.stream_sync()
    words = int(d_total.download(np.uint64, 2)[0])
    d_packed = al(2 * words)
    pack = XM.motion_params(d_mv=d_out.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_packed.ptr, d_total=d_total.ptr, width=w, height=h, cap_words=words)
    unpack = XM.motion_params(d_mv=d_mv2.ptr, d_level=d_level2.ptr, d_ctu=d_ctu.ptr, d_stream=d_packed.ptr, width=w, height=h, cap_words=words)
    codec.motion_pack_dev(pack)
    enc0 = XE.entropy_motion_params(d_ctu=d_ctu.ptr, d_words=d_packed.ptr, d_coded=d_coded.ptr, d_total=d_total.ptr, width=w, height=h, in_words=words)
    XE.entropy_encode_motion_dev(codec, enc0)
    codec.stream_sync()
    coded_words = int(d_total.download(np.uint64, 2)[0])
    d_stream = al(2 * coded_words + 16)
    enc = XE.entropy_motion_params(d_ctu=d_ctu.ptr, d_words=d_packed.ptr, d_coded=d_coded.ptr, d_stream=d_stream.ptr, d_total=d_total.ptr, width=w, height=h,
                                   in_words=words, cap_words=coded_words)
    dec = XE.entropy_motion_params(d_ctu=d_ctu2.ptr, d_words=d_words2.ptr, d_coded=d_coded.ptr, d_stream=d_stream.ptr, d_status=d_status.ptr, width=w, height=h,
                                   cap_words=coded_words)
    rec = XM.motion_params(d_mv=d_mv2.ptr, d_level=d_level2.ptr, d_ctu=d_ctu2.ptr, d_stream=d_words2.ptr, width=w, height=h, cap_words=256 * n_ctu)

    # one pass, checked against the reference and against the dense field
    XE.entropy_encode_motion_dev(codec, enc)
    XE.entropy_decode_motion_dev(codec, dec)
    codec.motion_reconstruct_dev(rec)
    codec.stream_sync()
    ctu, packed = d_ctu.download(np.uint8, 32 * n_ctu).view(M.CTU_DTYPE), d_packed.download(np.uint16, words)
    coded, stream = d_coded.download(np.uint8, 32 * n_ctu).view(EM.CODED_DTYPE), d_stream.download(np.uint16, coded_words)
    want, want_stream, want_total = EM.encode(ctu, packed, w, h)
    assert np.array_equal(coded, want) and np.array_equal(stream, want_stream) and int(want_total[0]) == coded_words, "encode differs from the reference"
    ctu2, status = d_ctu2.download(np.uint8, 32 * n_ctu).view(M.CTU_DTYPE), d_status.download(np.uint8, n_ctu)
    assert not status.any() and all(np.array_equal(ctu2[f], ctu[f]) for f in M.CTU_DTYPE.names if f != "offset"), "decode does not return pack's records"
    mv2, level2 = d_mv2.download(np.uint8, 8 * nb).view(M.ME_DTYPE), d_level2.download(np.uint8, nb)
    assert np.array_equal(mv2["mvx"], out["mvx"]) and np.array_equal(mv2["mvy"], out["mvy"]) and not mv2["cost"].any() and np.array_equal(level2, level)
    parts, bits, n_bytes = int(ctu["parts"].sum()), int(ctu["bits"].sum()), int(coded["n_bytes"].sum())
    assert int((coded["ctx_bins"] + coded["bypass_bins"]).sum()) == bits
    packed_bytes = 32 * n_ctu + 2 * words
    say("\n%d x %d: %d blocks, %d CTUs (%d x %d, %d reconstruct steps); the decided field of tools/gpu_motion_pack.py (lambda_q4 %d), %d partitions"
        % (w, h, nb, n_ctu, cw, ch, cw + 2 * (ch - 1), LAMBDA, parts))
    say("coded records, stream and totals equal tests/_entropy_motion_ref.py's; decode returns pack's records and differences; reconstruct returns d_out's vectors and d_level")
    say("bits of the pack records (= context + bypass bins, exactly) %d = %.0f bytes; coded bytes %d: %.3f of the estimate; %d CTUs of %d are 0 bytes, the longest %d"
        % (bits, bits / 8, n_bytes, n_bytes / (bits / 8), int((coded["n_bytes"] == 0).sum()), n_ctu, int(coded["n_bytes"].max())))
    say("packed records + stream %d bytes (%d + %d); coded records + words %d bytes (%d + %d): %.3f; the coded words alone against the packed stream alone %.3f"
        % (packed_bytes, 32 * n_ctu, 2 * words, 32 * n_ctu + 2 * coded_words, 32 * n_ctu, 2 * coded_words, (32 * n_ctu + 2 * coded_words) / packed_bytes,
           coded_words / max(1, words)))

    # the per-CTU restart: the whole frame as one chain, contexts carried over, one termination
    bw, bh = w // 8, h // 8
    bins = []
    for c in range(n_ctu):
        off, n = int(ctu["offset"][c]), int(ctu["n_words"][c])
        bins += EM.ctu_bins(bw, bh, c % cw, c // cw, int(ctu["head_mask"][c]), EM.true_diffs(packed[off:off + n]))
    one = len(ER.code_bins(bins, [int(x) for x in EM.default_init()]))
    say("the frame as ONE chain on the CPU (contexts carried from CTU to CTU, one termination): %d bytes; the independent substreams are %.3f of it"
        % (one, n_bytes / max(1, one)))

    calls = {"pack": lambda: codec.motion_pack_dev(pack), "unpack": lambda: codec.motion_unpack_dev(unpack),
             "encode, count-only": lambda: XE.entropy_encode_motion_dev(codec, enc0), "encode": lambda: XE.entropy_encode_motion_dev(codec, enc),
             "decode": lambda: XE.entropy_decode_motion_dev(codec, dec), "reconstruct": lambda: codec.motion_reconstruct_dev(rec)}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    host = dict(ctu=np.ones(32 * n_ctu, np.uint8), packed=np.ones(max(words, 1), np.uint16), coded=np.ones(32 * n_ctu, np.uint8), stream=np.ones(max(coded_words, 1), np.uint16))

    def copy(name, src, nbytes):
        if nbytes:
            codec._check(codec.L.xHipMemcpyD2H(codec.ctx, host[name].ctypes.data, src.ptr, nbytes), "xHipMemcpyD2H")

    def packed_copy():
        copy("ctu", d_ctu, 32 * n_ctu)
        last = host["ctu"].view(M.CTU_DTYPE)[-1]
        copy("packed", d_packed, 2 * (int(last["offset"]) + int(last["n_words"])))

    def coded_copy():
        copy("coded", d_coded, 32 * n_ctu)
        last = host["coded"].view(EM.CODED_DTYPE)[-1]
        copy("stream", d_stream, 2 * (int(last["offset"]) + int(last["n_words"])))

    hosts = {"host: packed records + stream": packed_copy, "host: coded records + words": coded_copy}

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
    assert np.array_equal(host["coded"].view(EM.CODED_DTYPE), want) and np.array_equal(host["stream"][:coded_words], want_stream)
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d back-to-back repetitions, all legs alternating; device legs by device events, host legs by the host's clock" % (ROUNDS, REPS))
    say("%-32s %10s %10s %10s" % ("leg", "us", "min us", "max us"))
    for k in ms:
        say("%-32s %10.1f %10.1f %10.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3))
    say("encode / pack = %.1f; count-only / encode = %.2f; decode / unpack = %.1f; reconstruct / unpack = %.1f, %.2f us per step of %d"
        % (t["encode"] / t["pack"], t["encode, count-only"] / t["encode"], t["decode"] / t["unpack"], t["reconstruct"] / t["unpack"],
           t["reconstruct"] * 1e3 / (cw + 2 * (ch - 1)), cw + 2 * (ch - 1)))
    say("coded copy / packed copy = %.3f" % (t["host: coded records + words"] / t["host: packed records + stream"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r30_entropy_motion.txt")
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
