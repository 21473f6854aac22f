#!/usr/bin/env python3
"""Timing of the adaptive loop filter at 3840 x 2176 (4K padded to whole CTUs), device events after warm-up, all in ONE process, the
legs alternating within every round, 10 % trimmed mean over the rounds:

  classify / stats / totals / decide / apply   xAlfClassifyGpu / xAlfStatsGpu / xAlfSumStatsGpu / xAlfDecideGpu / xAlfApplyGpu; stats and
                                               apply with the class map of classify and, "(inside)", with d_class == NULL
  sao stats / sao apply                        xSaoStatsGpu / xSaoApplyGpu on the same frame
  copy of a call's bytes                       this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) moving as many bytes as the call
                                               reads plus writes: m_Y is 256 bytes per tile, m_Y + m_C 384, a class map 16, a CTU's
                                               statistics 9432, the totals 18864

"of copy" = copy time / call time.  No rate is a pass / fail condition.
The source is a smooth field with edges and Gaussian noise, the decoded frame its 5-tap blur plus +-3 noise (the `blur` recipe of
tests/_alf_ref.py at frame size).  The filters are solved on the host in float64 from the totals the device sums, as an encoder would:
one luma set, U's and V's solutions as the two chroma alternatives; the tool reports what the decision picks and the squared error
before and after apply.
Usage: gpu_alf.py [--out FILE]   (default profiles/r17_alf.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS, LAMBDA_Q4 = 20, 20, 37
WORDS = 2358


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def planes(rs, pw, ph, scale):
    """(org, dec) of one plane"""
    yy, xx = np.mgrid[0:ph, 0:pw] * scale
    ramp = 0.4 + 0.6 * xx / (pw * scale - 1)
    field = 40 * np.sin(xx / 7.0) * np.cos(yy / 11.0) + 25 * np.sin((xx + 2 * yy) / 17.0)
    edges = 22 * np.sign(np.sin((xx + yy) / 9.0)) + 18 * np.sign(np.sin((2 * xx - yy) / 13.0))
    org = np.clip(np.round(128 + ramp * (field + edges) + rs.normal(0.0, 6.0, (ph, pw))), 0, 255).astype(np.int64)
    big = np.pad(org, 1, mode="edge")
    dec = np.clip(((4 * org + big[1:-1, :-2] + big[1:-1, 2:] + big[:-2, 1:-1] + big[2:, 1:-1] + 4) >> 3) + rs.randint(-3, 4, (ph, pw)), 0, 255)
    return org.astype(np.uint8), dec.astype(np.uint8)


def tiles_of(y, u, v, rs):
    h, w = y.shape
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    c = np.stack([u, v], axis=-1).reshape(h // 16, 8, w // 16, 16).transpose(0, 2, 1, 3)
    t[:, :, 256:384] = c.reshape(h // 16, w // 16, 128)
    return t.ravel()


def solve_record(rec, n):
    """coefficients of one record of totals: lstsq(A + 1e-3 I, b), 7 fractional bits"""
    rec = np.asarray(rec, np.float64)
    a = np.zeros((n, n))
    iu = np.triu_indices(n)
    a[iu] = rec[2 + n:]
    a = a + np.triu(a, 1).T
    x = np.linalg.lstsq(a + 1e-3 * np.eye(n), rec[2:2 + n], rcond=None)[0]
    return np.clip(np.round(128 * x), -128, 127).astype(np.int64)


def squared_error(a, b):
    """over m_Y and m_C of two tile arrays"""
    d = a.reshape(-1, 512)[:, :384].astype(np.int64) - b.reshape(-1, 512)[:, :384].astype(np.int64)
    return int((d * d).sum())


def measure(codec, ev, w, h, say):
    nt, tile_bytes, n, nb = (w // 16) * (h // 16), w * h * 2, codec.ctu_count(w, h), (w // 4) * (h // 4)
    rs = np.random.RandomState(0x266)
    pairs = [planes(rs, w, h, 1), planes(rs, w // 2, h // 2, 2), planes(rs, w // 2, h // 2, 2)]
    org_h, dec_h = tiles_of(*[p[0] for p in pairs], rs), tiles_of(*[p[1] for p in pairs], rs)
    org, dec, out, sao_out = (codec.alloc(tile_bytes) for _ in range(4))
    cls, stats, stats2, total, ctrl = codec.alloc(nb), codec.alloc(n * WORDS * 4), codec.alloc(n * WORDS * 4), codec.alloc(WORDS * 8), codec.alloc(3 * n)
    sao_stats, sao_par = codec.alloc(n * 1152), codec.alloc(n * 24)
    org.upload(org_h)
    dec.upload(dec_h)
    # one pass as an encoder runs it: classify, statistics, totals, the solve on the host, decision, apply
    codec.alf_classify_dev(dec.ptr, w, h, cls.ptr)
    codec.alf_stats_dev(org.ptr, dec.ptr, w, h, cls.ptr, stats.ptr)
    codec.alf_stats_dev(org.ptr, dec.ptr, w, h, 0, stats2.ptr)
    codec.alf_sum_stats_dev(stats.ptr, n, 0, total.ptr)
    codec.stream_sync()
    assert np.array_equal(stats.download(np.int32, n * WORDS), stats2.download(np.int32, n * WORDS)), "classifying inside changes the statistics"
    tot = total.download(np.int64, WORDS)
    luma_coef = np.stack([solve_record(tot[92 * k:92 * k + 92], 12) for k in range(25)])
    luma_h, chroma_h = codec.alf_pack_filters(luma_coef[None], None, np.stack([solve_record(tot[2300:2329], 6), solve_record(tot[2329:], 6)]), None)
    luma, chroma = codec.alloc(600), codec.alloc(32)
    luma.upload(luma_h)
    chroma.upload(chroma_h)
    codec.alf_decide_dev(stats.ptr, n, luma.ptr, 1, chroma.ptr, 2, LAMBDA_Q4, ctrl.ptr)
    codec.alf_apply_dev(dec.ptr, w, h, cls.ptr, luma.ptr, 1, chroma.ptr, 2, ctrl.ptr, out.ptr)
    codec.sao_search_dev(org.ptr, dec.ptr, w, h, LAMBDA_Q4, sao_par.ptr)
    codec.stream_sync()
    picks, out_h = ctrl.download(np.uint8, 3 * n).reshape(n, 3), out.download(np.uint8, tile_bytes)
    say("\n%d x %d (%d tiles, %d CTUs, %d class bytes): classes in use %d of 25; the decision filters %d / %d / %d of the CTUs' Y / U / V (U picks alternative "
        "%s, V %s); squared error %d -> %d" % (w, h, nt, n, nb, int((tot[0:2300:92] != 0).sum()), int((picks[:, 0] != 0).sum()), int((picks[:, 1] != 0).sum()),
                                              int((picks[:, 2] != 0).sum()), np.bincount(picks[:, 1], minlength=3)[1:3].tolist(),
                                              np.bincount(picks[:, 2], minlength=3)[1:3].tolist(), squared_error(org_h, dec_h), squared_error(org_h, out_h)))

    moved = {"classify": nt * 272, "stats": nt * 784 + n * WORDS * 4, "stats (inside)": nt * 768 + n * WORDS * 4, "totals": n * WORDS * 4 + WORDS * 8,
             "decide": n * WORDS * 4 + 3 * n, "apply": nt * 784, "apply (inside)": nt * 768, "sao stats": nt * 768, "sao apply": nt * 768}
    calls = {"classify": lambda: codec.alf_classify_dev(dec.ptr, w, h, cls.ptr),
             "stats": lambda: codec.alf_stats_dev(org.ptr, dec.ptr, w, h, cls.ptr, stats.ptr),
             "stats (inside)": lambda: codec.alf_stats_dev(org.ptr, dec.ptr, w, h, 0, stats.ptr),
             "totals": lambda: codec.alf_sum_stats_dev(stats.ptr, n, 0, total.ptr),
             "decide": lambda: codec.alf_decide_dev(stats.ptr, n, luma.ptr, 1, chroma.ptr, 2, LAMBDA_Q4, ctrl.ptr),
             "apply": lambda: codec.alf_apply_dev(dec.ptr, w, h, cls.ptr, luma.ptr, 1, chroma.ptr, 2, ctrl.ptr, out.ptr),
             "apply (inside)": lambda: codec.alf_apply_dev(dec.ptr, w, h, 0, luma.ptr, 1, chroma.ptr, 2, ctrl.ptr, out.ptr),
             "sao stats": lambda: codec.sao_stats_dev(org.ptr, dec.ptr, w, h, sao_stats.ptr),
             "sao apply": lambda: codec.sao_apply_dev(dec.ptr, w, h, sao_par.ptr, sao_out.ptr)}
    half = (max(moved.values()) // 2 + 15) & ~15
    ca, cb = codec.alloc(half), codec.alloc(half)
    codec.fill_residual_dev(ca.ptr, half // 2, 0x71)
    for k, b in list(moved.items()):
        calls["copy: " + k] = lambda nbytes=b // 2: codec.mem_ceiling_dev(0, ca.ptr, cb.ptr, nbytes & ~15)

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
    say("%-26s %9s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "GB/s", "of copy"))
    for k in calls:
        name = k[6:] if k.startswith("copy: ") else k
        of = "" if k.startswith("copy: ") else "%9.3f" % (t["copy: " + k] / t[k])
        say("%-26s %9.2f %9.2f %9.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, moved[name] / t[k] / 1e6, of))
    say("alf stats / sao stats %.2f, alf apply / sao apply %.2f" % (t["stats"] / t["sao stats"], t["apply"] / t["sao apply"]))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r17_alf.txt")
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
