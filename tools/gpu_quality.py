#!/usr/bin/env python3
"""Timing of frame quality at 3840 x 2176 (4K padded to whole CTUs), all in ONE process.  The device legs are timed by device events
after warm-up, alternating within every round, 10 % trimmed mean over the rounds:

  sse + ssim, ssim, sse   xQualityStatsGpu with both flags, with X266_QUALITY_SSIM and with X266_QUALITY_SSE alone: the CTU records (one
                          launch, a workgroup per CTU) and the totals (one workgroup), as a caller pays for them
  read 2 x 384 / 512      this box's read stream (xHipMemCeilingDev X266_MEM_READ, the diagnostic stream kernel) over as many bytes as the
                          call uses of the two frames (m_Y + m_C: 384 bytes per tile) and as the two frames hold (512 per tile)

and against them what the tools and examples did for the same number until now, timed by the host clock around work that ends in the
copies' synchronisation:

  host sse                two xConvOutput420Dev, two device-to-host copies of the planes (pageable memory) and numpy's sum of squares

"of read" = read-stream time of 2 x 384 bytes per tile / call time.  No rate is a pass / fail condition.
The source is the smooth field with edges, flat patches and noise of tools/gpu_aq.py, the decoded frame the same with a +-3 perturbation;
the tool checks the device's squared error against numpy's, exactly, and the frame SSIM against the float64 formula over every window.
Usage: gpu_quality.py [--out FILE]   (default profiles/r25_quality.txt)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.quality as Q  # noqa: E402

ROUNDS, REPS, HOST_ROUNDS = 20, 20, 7


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def frames(w, h):
    """(source tiles, decoded tiles, their planes)"""
    import _aq_ref as A
    from gpu_aq import plane
    rs = np.random.RandomState(0x266)
    src = [plane(rs, w, h, 1), plane(rs, w // 2, h // 2, 2), plane(rs, w // 2, h // 2, 2)]
    dec = [np.clip(p.astype(np.int64) + rs.randint(-3, 4, p.shape), 0, 255).astype(np.uint8) for p in src]
    return A.tiles_from_planes(*src, 7), A.tiles_from_planes(*dec, 8), src, dec


def float_ssim(a, b):
    """the mean of the float64 formula over every window of a plane pair"""
    import _quality_ref as R
    s1, s2, ss, s12 = [x.astype(np.float64) for x in R.window_sums(a, b)]
    var, covar = 64.0 * ss - s1 * s1 - s2 * s2, 64.0 * s12 - s1 * s2
    return float(((2.0 * s1 * s2 + R.C1) * (2.0 * covar + R.C2) / ((s1 * s1 + s2 * s2 + R.C1) * (var + R.C2))).mean())


def measure(codec, ev, w, h, say):
    nt, n = (w // 16) * (h // 16), codec.ctu_count(w, h)
    src_tiles, dec_tiles, src_planes, dec_planes = frames(w, h)
    d_src, d_dec, d_ctu, d_total = codec.alloc(nt * 512), codec.alloc(nt * 512), codec.alloc(n * 48), codec.alloc(64)
    d_src.upload(src_tiles)
    d_dec.upload(dec_tiles)
    params = {name: Q.quality_params(d_src=d_src.ptr, d_dec=d_dec.ptr, d_ctu=d_ctu.ptr, d_total=d_total.ptr, width=w, height=h, flags=flags)
              for name, flags in (("sse + ssim", 3), ("ssim", 2), ("sse", 1))}

    # what it computes, against numpy
    codec.quality_stats_dev(params["sse + ssim"])
    codec.stream_sync()
    total = d_total.download(np.int64, 8)
    want_sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(src_planes, dec_planes)]
    assert total[:3].tolist() == want_sse, "the squared error differs from numpy's: %s, %s" % (total[:3].tolist(), want_sse)
    psnr, ssim = Q.from_totals(total, w, h)
    want_ssim = [float_ssim(a, b) for a, b in zip(src_planes, dec_planes)]
    assert max(abs(g - e) for g, e in zip(ssim, want_ssim)) <= 4 * 2.0 ** -30, "the frame SSIM differs from the float64 formula: %s, %s" % (ssim, want_ssim)
    say("\n%d x %d (%d tiles, %d CTUs), source against source +-3: PSNR Y %.3f U %.3f V %.3f all %.3f dB, SSIM Y %.6f U %.6f V %.6f"
        % (w, h, nt, n, psnr[0], psnr[1], psnr[2], psnr[3], ssim[0], ssim[1], ssim[2]))
    say("squared error %s = numpy's; frame SSIM within 4 * 2^-30 of the float64 formula over all %d + 2 x %d windows" % (total[:3].tolist(), total[6], total[7]))

    calls = {name: (lambda p=p: codec.quality_stats_dev(p)) for name, p in params.items()}
    moved = {name: 2 * nt * 384 + 2 * n * 48 + 64 for name in calls}
    sums = codec.alloc(2 * nt * 512 // 2048 * 4 + 16)
    # the two frames are two allocations: one read stream over each, back to back
    calls["read 2 x 384 B / tile"] = lambda: (codec.mem_ceiling_dev(1, d_src.ptr, sums.ptr, nt * 384), codec.mem_ceiling_dev(1, d_dec.ptr, sums.ptr, nt * 384))
    calls["read 2 x 512 B / tile"] = lambda: (codec.mem_ceiling_dev(1, d_src.ptr, sums.ptr, nt * 512), codec.mem_ceiling_dev(1, d_dec.ptr, sums.ptr, nt * 512))
    moved["read 2 x 384 B / tile"], moved["read 2 x 512 B / tile"] = 2 * nt * 384, 2 * nt * 512

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

    # the host's way: planes out of the tiles, both frames to the host, numpy
    planes = [[codec.alloc(w * h), codec.alloc(w * h // 4), codec.alloc(w * h // 4)] for _ in range(2)]

    def host_sse():
        got = []
        for d_tiles, (dy, du, dv) in zip((d_src, d_dec), planes):
            codec.conv_output_420_dev(d_tiles.ptr, dy.ptr, w, du.ptr, dv.ptr, w // 2, w, h)
        for dy, du, dv in planes:
            got.append([dy.download(np.uint8, w * h), du.download(np.uint8, w * h // 4), dv.download(np.uint8, w * h // 4)])
        out = []
        for a, b in zip(got[0], got[1]):
            d = a.astype(np.int32) - b.astype(np.int32)
            out.append(int((d * d).sum(dtype=np.int64)))
        return out

    assert host_sse() == want_sse
    host = []
    for _ in range(HOST_ROUNDS):
        t0 = time.perf_counter()
        host_sse()
        host.append((time.perf_counter() - t0) * 1e3)
    t["host sse"], ms["host sse"], moved["host sse"] = trimmed_mean(host), host, 2 * nt * 512 + 2 * (w * h * 3 // 2) * 2

    say("device legs: 10 %% trimmed mean of %d rounds of %d back-to-back calls, all legs alternating; host sse: %d runs by the host clock" % (ROUNDS, REPS, HOST_ROUNDS))
    say("GB/s over the bytes a leg reads and writes on the device")
    say("%-24s %10s %10s %10s %9s %9s" % ("leg", "us", "min us", "max us", "GB/s", "of read"))
    for k in list(calls) + ["host sse"]:
        of = "" if k.startswith("read") else "%9.4f" % (t["read 2 x 384 B / tile"] / t[k])
        say("%-24s %10.2f %10.2f %10.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, moved[k] / t[k] / 1e6, of))
    say("host sse / sse %.0fx, host sse / sse + ssim %.0fx; sse + ssim / sse %.2fx" % (t["host sse"] / t["sse"], t["host sse"] / t["sse + ssim"], t["sse + ssim"] / t["sse"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r25_quality.txt")
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
