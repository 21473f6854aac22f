#!/usr/bin/env python3
"""Timing of sample adaptive offset at 1080p (1920 x 1088: the calls take multiples of 16) and 4K (3840 x 2160), device events after
warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  stats / decide / search / apply      xSaoStatsGpu / xSaoDecideGpu / xSaoSearchGpu (without d_stats) / xSaoApplyGpu
  copy of a call's bytes               this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) moving as many bytes as the call:
                                       stats and search read m_Y + m_C of two frames (768 bytes per tile; the copy reads 384 and
                                       writes 384), apply reads and writes 384 per tile, decide reads 1152 bytes per CTU

"of copy" = copy time / call time.  Also: search / (stats + decide back to back).  No rate is a pass / fail condition.
The source is a sinusoid with +-8 noise; the decoded frame is over-sharpened along one EO class per CTU, has a band shifted by 3, or
differs by +-1 noise, CTU by CTU (the recipe of tests/_sao_ref.py at frame size), so every type is decided and applied.
Usage: gpu_sao.py [--out FILE]   (default profiles/r14_sao.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS, LAMBDA_Q4 = 20, 50, 37


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def planes(rs, pw, ph, edge):
    """(org, dec) of one plane, the treatment changing from CTU to CTU"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    scale = 64 // edge
    org = np.clip(128 + (70 * np.sin(xx * scale / 9.0) * np.cos(yy * scale / 13.0)).astype(np.int64) + rs.randint(-8, 9, (ph, pw)), 0, 255)
    big = np.pad(org, 1, mode="edge")
    shifts = (((0, -1), (0, 1)), ((-1, 0), (1, 0)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1)))       # (dy, dx) of a and b per EO class
    sharp = [np.clip(2 * org - ((big[1 + a[0]:1 + a[0] + ph, 1 + a[1]:1 + a[1] + pw] + 2 * org + big[1 + b[0]:1 + b[0] + ph, 1 + b[1]:1 + b[1] + pw] + 2) >> 2), 0, 255)
             for a, b in shifts]
    what = ((yy // edge) * ((pw + edge - 1) // edge) + xx // edge) % 6
    dec = np.select([what == k for k in range(4)] + [what == 4], sharp + [np.where((org >= 100) & (org <= 131), org - 3, org)],
                    np.clip(org + rs.randint(-1, 2, (ph, pw)), 0, 255))
    return org.astype(np.uint8), dec.astype(np.uint8)


def tiles_of(y, u, v, rs):
    h, w = y.shape
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    c = np.stack([u, v], axis=-1).reshape(h // 16, 8, w // 16, 16).transpose(0, 2, 1, 3)
    t[:, :, 256:384] = c.reshape(h // 16, w // 16, 128)
    return t.ravel()


def measure(codec, ev, w, h, say):
    nt, tile_bytes, n = (w // 16) * (h // 16), w * h * 2, codec.ctu_count(w, h)
    rs = np.random.RandomState(0x266)
    pairs = [planes(rs, w, h, 64), planes(rs, w // 2, h // 2, 32), planes(rs, w // 2, h // 2, 32)]
    org_h, dec_h = tiles_of(*[p[0] for p in pairs], rs), tiles_of(*[p[1] for p in pairs], rs)
    org, dec, out = codec.alloc(tile_bytes), codec.alloc(tile_bytes), codec.alloc(tile_bytes)
    stats, par, par2 = codec.alloc(n * 1152), codec.alloc(n * 24), codec.alloc(n * 24)
    org.upload(org_h)
    dec.upload(dec_h)
    # the fused search is the pair (on this frame; the tests hold the statement)
    codec.sao_stats_dev(org.ptr, dec.ptr, w, h, stats.ptr)
    codec.sao_decide_dev(stats.ptr, n, LAMBDA_Q4, par.ptr)
    codec.sao_search_dev(org.ptr, dec.ptr, w, h, LAMBDA_Q4, par2.ptr)
    codec.sao_apply_dev(dec.ptr, w, h, par.ptr, out.ptr)
    codec.stream_sync()
    rec = par.download(np.uint8, n * 24).reshape(n, 3, 8)
    assert np.array_equal(par2.download(np.uint8, n * 24).reshape(n, 3, 8), rec), "the fused search differs from the pair"
    changed = out.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384] != dec_h.reshape(-1, 512)[:, :384]
    say("\n%d x %d (%d tiles, %d CTUs): luma off / BO / EO %s, chroma %s; %.1f %% of the samples change" % (
        w, h, nt, n, np.bincount(rec[:, 0, 0], minlength=3)[:3].tolist(), np.bincount(rec[:, 1, 0], minlength=3)[:3].tolist(), 100.0 * changed.mean()))

    moved = {"stats": nt * 768, "decide": n * 1152, "search": nt * 768, "apply": nt * 768}     # bytes a call reads plus writes
    calls = {"stats": lambda: codec.sao_stats_dev(org.ptr, dec.ptr, w, h, stats.ptr),
             "decide": lambda: codec.sao_decide_dev(stats.ptr, n, LAMBDA_Q4, par.ptr),
             "search": lambda: codec.sao_search_dev(org.ptr, dec.ptr, w, h, LAMBDA_Q4, par2.ptr),
             "apply": lambda: codec.sao_apply_dev(dec.ptr, w, h, par.ptr, out.ptr)}
    ca, cb = codec.alloc(nt * 384), codec.alloc(nt * 384)
    codec.fill_residual_dev(ca.ptr, nt * 192, 0x71)
    for k, b in list(moved.items()):
        calls["copy of %s's bytes" % k] = lambda nbytes=b // 2: codec.mem_ceiling_dev(0, ca.ptr, cb.ptr, nbytes & ~15)

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
        name = k.split()[2][:-2] if k.startswith("copy") else k
        of = "" if k.startswith("copy") else "%9.3f" % (t["copy of %s's bytes" % k] / t[k])
        say("%-26s %9.2f %9.2f %9.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, moved[name] / t[k] / 1e6, of))
    say("search / (stats + decide back to back) %.3f" % (t["search"] / (t["stats"] + t["decide"])))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r14_sao.txt")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    for w, h in ((1920, 1088), (3840, 2160)):
        measure(codec, ev, w, h, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
