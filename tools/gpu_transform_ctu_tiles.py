#!/usr/bin/env python3
"""Timing of the mixed transform set per CTU from and into tiled frames (xTransformCtuFromTilesDev / xTransformCtuToTilesDev)
-- device events after warm-up, all in ONE process, the calls alternating within every round.
Usage: gpu_transform_ctu_tiles.py [W]  (default: 32768, a W x W frame).

Algorithmic bytes are 24 KiB per full 64x64 CTU in each direction: forward 12 KiB of cur + pred read (m_Y and m_C of 16 tiles
each), 12 KiB of coefficients written; inverse 12 KiB of coefficients + 6 KiB of pred read, 6 KiB written.  Next to them: the
copy stream of the same bytes (xHipMemCeilingDev X266_MEM_COPY of 12 KiB per CTU: a copy of B bytes moves 2 B), the one-launch
tile transform xTransformTilesDev over the equivalent CTU-ordered residual buffer (the same 24 KiB per CTU), and, on the all-32
mix, the DCT32 CTU calls (xDct32FwdCtuFromTilesDev / xDct32InvCtuToTilesDev).  "of copy" = copy time / call time.
Three class mixes: every region (DCT-II, 32); class bytes uniform over 0..15; an encoder-like mix (a third 32x32, a third 16x16,
a sixth 8x8, a sixth 4x4, types uniform).  Then per-call latency at 3840x2160 and 7680x4320 (encoder-like mix)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS = 7, 10
CTU_BYTES = 24576


def mixes(n, seed):
    r = np.random.default_rng(seed)
    sizes = r.choice([3, 3, 2, 2, 1, 0], 6 * n)
    return {"all (DCT-II, 32)": np.full(6 * n, 3, np.uint8),
            "uniform 0..15": r.integers(0, 16, 6 * n).astype(np.uint8),
            "encoder-like": (r.integers(0, 4, 6 * n) * 4 + sizes).astype(np.uint8)}


def main(argv):
    side = int(argv[0]) if argv else 32768
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    print("device: %s" % (codec.device_info(),))

    def timed(fn, reps=REPS):
        codec.event_record(ev[0])
        for _ in range(reps):
            fn()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / reps

    w = h = side
    n = ((w + 63) // 64) * ((h + 63) // 64)
    tb = w * h * 2
    d_cur, d_pred, d_rec = codec.alloc(tb), codec.alloc(tb), codec.alloc(tb)
    d_coef, d_res = codec.alloc(n * 12288), codec.alloc(n * 12288)
    d_src, d_dst = codec.alloc(n * 12288), codec.alloc(n * 12288)
    for i, d in enumerate((d_cur, d_pred, d_rec)):
        codec.fill_residual_dev(d.ptr, tb // 2, 0x90 + i)
    codec.fill_residual_dev(d_src.ptr, n * 6144, 0x93)
    codec.fill_residual_dev(d_res.ptr, n * 6144, 0x94)
    codec.stream_sync()
    d_cls = {k: codec.alloc(6 * n) for k in mixes(1, 0)}
    for k, v in mixes(n, 0x95).items():
        d_cls[k].upload(v)
    algo = n * CTU_BYTES
    calls = {"copy of the same bytes": lambda: codec.mem_ceiling_dev(0, d_src.ptr, d_dst.ptr, n * 12288)}
    for k in d_cls:
        c = d_cls[k].ptr
        calls["fwd " + k] = lambda c=c: codec.transform_ctu_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, c, d_coef.ptr)
        calls["inv " + k] = lambda c=c: codec.transform_ctu_to_tiles_dev(d_coef.ptr, c, d_pred.ptr, w, h, d_rec.ptr)
        calls["tiles fwd " + k] = lambda c=c: codec.transform_tiles_dev(0, d_res.ptr, d_coef.ptr, 6 * n, 0, c)
        calls["tiles inv " + k] = lambda c=c: codec.transform_tiles_dev(1, d_coef.ptr, d_res.ptr, 6 * n, 0, c)
    calls["dct32 ctu fwd"] = lambda: codec.dct32_fwd_ctu_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, d_coef.ptr)
    calls["dct32 ctu inv"] = lambda: codec.dct32_inv_ctu_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_rec.ptr)
    for fn in calls.values():                                           # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print("\n%d x %d (%d CTUs, %d algorithmic bytes per call), median of %d rounds x %d calls, calls alternating"
          % (w, h, n, algo, ROUNDS, REPS))
    print("%-34s %9s %9s %9s %8s %8s %8s" % ("call", "ms", "min ms", "max ms", "spread", "TB/s", "of copy"))
    for k in calls:
        print("%-34s %9.4f %9.4f %9.4f %7.1f%% %8.3f %8.3f" % (k, med[k], min(ms[k]), max(ms[k]),
              100.0 * (max(ms[k]) - min(ms[k])) / med[k], algo / (med[k] * 1e-3) / 1e12, med["copy of the same bytes"] / med[k]))
    a32 = "all (DCT-II, 32)"
    print("all-32 mix against the DCT32 CTU calls: fwd %.4f x, inv %.4f x"
          % (med["fwd " + a32] / med["dct32 ctu fwd"], med["inv " + a32] / med["dct32 ctu inv"]))
    for k in d_cls:
        print("%-20s CTU call / tile transform of the residual buffer: fwd %.4f x, inv %.4f x"
              % (k, med["fwd " + k] / med["tiles fwd " + k], med["inv " + k] / med["tiles inv " + k]))
    for d in (d_cur, d_pred, d_rec, d_coef, d_res, d_src, d_dst, *d_cls.values()):
        d.free()

    print("\nper-call latency, encoder-like mix (median of %d rounds of %d calls)" % (ROUNDS, REPS))
    for w, h in ((3840, 2160), (7680, 4320)):
        n = ((w + 63) // 64) * ((h + 63) // 64)
        dc, dp, dr, dz = codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(w * h * 2), codec.alloc(n * 12288)
        for i, d in enumerate((dc, dp)):
            codec.fill_residual_dev(d.ptr, w * h, 0xA0 + i)
        dk = codec.alloc(6 * n)
        dk.upload(mixes(n, 0xA2)["encoder-like"])
        f = lambda: codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
        g = lambda: codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dr.ptr)
        for _ in range(3):
            f()
            g()
        codec.stream_sync()
        tf, ti = [], []
        for _ in range(ROUNDS):
            tf.append(timed(f))
            ti.append(timed(g))
        print("%5d x %4d (%5d CTUs): forward %7.2f us, inverse %7.2f us" % (w, h, n, statistics.median(tf) * 1e3, statistics.median(ti) * 1e3))
        for d in (dc, dp, dr, dz, dk):
            d.free()
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
