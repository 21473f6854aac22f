#!/usr/bin/env python3
"""Timing of in-loop deblocking on a 4K frame (3840 x 2160), device events after warm-up, all in ONE process, the legs alternating
within every round, 10 % trimmed mean over the rounds:

  luma / chroma / fused, out of place and in place     xDeblockLumaGpu / ChromaGpu / Gpu with every side array given
  copy of the luma / chroma / fused bytes              this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) of the bytes a call
                                                       reads once and writes once: 256 (m_Y), 128 (m_C), 384 per tile

"of copy" = copy time / call time.  Ratios a reviewer asks for: in place / out of place, fused / (luma + chroma back to back).
The frame is per-block levels with a ramp and +-2 noise (uniform noise would switch nearly every segment off), mixed classes,
a third of the regions intra, half of them coded, qp 20..51, vectors that differ at a quarter of the blocks.
Usage: gpu_deblock.py [W H] [--out FILE]   (default 3840 2160, profiles/r13_deblock.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS = 20, 50


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def blocky_plane(rs, pw, ph):
    levels = np.repeat(np.repeat(rs.randint(104, 152, (ph // 8, pw // 8)), 8, 0), 8, 1)
    yy, xx = np.mgrid[0:ph, 0:pw]
    return np.clip(levels + (xx + 2 * yy) // 64 % 32 + rs.randint(-2, 3, (ph, pw)), 0, 255).astype(np.uint8)


def tiles_of(y, u, v, rs):
    h, w = y.shape
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    c = np.stack([u, v], axis=-1).reshape(h // 16, 8, w // 16, 16).transpose(0, 2, 1, 3)
    t[:, :, 256:384] = c.reshape(h // 16, w // 16, 128)
    return t.ravel()


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r13_deblock.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    w, h = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3840, 2160)
    assert w % 16 == 0 and h % 16 == 0
    lines = []

    def say(s=""):
        print(s)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    nb, nt, tile_bytes, n = (w // 8) * (h // 8), (w // 16) * (h // 16), w * h * 2, codec.ctu_count(w, h) * 6
    rs = np.random.RandomState(0x266)
    frame_h = tiles_of(blocky_plane(rs, w, h), blocky_plane(rs, w // 2, h // 2), blocky_plane(rs, w // 2, h // 2), rs)
    rec = np.zeros((nb, 4), np.int16)
    rec[:, :2] = np.where(rs.randint(0, 4, (nb, 1)) == 0, rs.randint(-16, 17, (nb, 2)), 5)
    host = [rs.randint(0, 16, n).astype(np.uint8), np.where(rs.randint(0, 3, n) == 0, 1, 0).astype(np.uint8),
            (rs.randint(0, 2, n) * rs.randint(1, 1025, n)).astype(np.uint32), rs.randint(20, 52, n).astype(np.uint8), rec]
    side = []
    for a in host:
        side.append(codec.alloc(a.nbytes))
        side[-1].upload(a)
    params = codec.deblock_params(*[b.ptr for b in side], 0, 0, 0)
    src, work, dst = codec.alloc(tile_bytes), codec.alloc(tile_bytes), codec.alloc(tile_bytes)
    src.upload(frame_h)
    work.upload(frame_h)
    fns = {"luma": codec.deblock_luma_dev, "chroma": codec.deblock_chroma_dev, "fused": codec.deblock_dev}
    # the fused call is the pair, and in place is out of place (on this frame; the tests hold the statement)
    codec.deblock_luma_dev(src.ptr, w, h, params, dst.ptr)
    codec.deblock_chroma_dev(src.ptr, w, h, params, dst.ptr)
    codec.deblock_dev(src.ptr, w, h, params, work.ptr)
    codec.stream_sync()
    pair = dst.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384].copy()
    assert np.array_equal(work.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384], pair), "the fused call differs from the pair"
    work.upload(frame_h)
    codec.deblock_dev(work.ptr, w, h, params, work.ptr)
    codec.stream_sync()
    assert np.array_equal(work.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384], pair), "in place differs from out of place"
    say("%.1f %% of the luma and %.1f %% of the chroma samples change" % (
        100.0 * (pair[:, :256] != frame_h.reshape(-1, 512)[:, :256]).mean(), 100.0 * (pair[:, 256:] != frame_h.reshape(-1, 512)[:, 256:384]).mean()))

    per_tile = {"luma": 256, "chroma": 128, "fused": 384}                # bytes read once and written once per tile
    calls = {}
    for p in per_tile:
        calls["out of place " + p] = lambda p=p: fns[p](src.ptr, w, h, params, dst.ptr)
        calls["in place     " + p] = lambda p=p: fns[p](work.ptr, w, h, params, work.ptr)   # filters its own output again: same traffic
    ca, cb = codec.alloc(nt * 384), codec.alloc(nt * 384)
    codec.fill_residual_dev(ca.ptr, nt * 192, 0x71)
    for p, b in per_tile.items():
        calls["copy of the %s bytes" % p] = lambda nbytes=nt * b: codec.mem_ceiling_dev(0, ca.ptr, cb.ptr, nbytes & ~15)

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
    say("\n%d x %d (%d tiles): 10 %% trimmed mean of %d rounds of %d calls, all legs alternating" % (w, h, nt, ROUNDS, REPS))
    say("%-26s %9s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "GB/s", "of copy"))
    for k in calls:
        p = k.split()[-2] if k.startswith("copy") else k.split()[-1]
        of = "" if k.startswith("copy") else "%9.3f" % (t["copy of the %s bytes" % p] / t[k])
        say("%-26s %9.2f %9.2f %9.2f %9.0f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, 2 * nt * per_tile[p] / t[k] / 1e6, of))
    for p in per_tile:
        say("%-6s: in place / out of place %.3f" % (p, t["in place     " + p] / t["out of place " + p]))
    for kind in ("out of place ", "in place     "):
        say("%s: fused / (luma + chroma back to back) %.3f" % (kind.strip(), t[kind + "fused"] / (t[kind + "luma"] + t[kind + "chroma"])))
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
