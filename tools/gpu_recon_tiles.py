#!/usr/bin/env python3
"""Timing of the reconstruction-into-tiles entry points (xReconLumaDev, xReconChromaDev, xDct32InvToTilesDev,
xDct32InvCtuToTilesDev): each call on a large frame, the two-call path it replaces, and this box's copy stream
(xHipMemCeilingDev X266_MEM_COPY) over the same algorithmic bytes -- device events after warm-up, all in ONE process,
alternating rounds.  Usage: gpu_recon_tiles.py [W H ...]  (default: 32768 32768 3840 2176).

Algorithmic bytes per pixel of the frame (w x h luma, 4:2:0): recon luma 4 (pred m_Y 1 + int16 residual 2 + m_Y 1), recon
chroma 2 (m_C 0.5 + U / V residual 1 + m_C 0.5), fused inverse 4 (coefficients 2 + m_Y 1 + 1), two-call luma 8 (inverse 2 + 2,
recon 4), whole CTU 6 (coefficients 3 + m_Y / m_C 1.5 + 1.5), its unfused path 12.  A copy of B bytes moves 2 B, so the
reference stream for a call of A bytes copies A / 2; "of copy" = copy time / call time."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import x266_amd  # noqa: E402

ROUNDS, REPS = 7, 20


def main(argv):
    sizes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or [(32768, 32768), (3840, 2176)]
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    print("device: %s" % (codec.device_info(),))
    for w, h in sizes:
        assert w % 64 == 0 and h % 64 == 0
        px = w * h
        n32, n_ctu = px // 1024, px // 4096
        pred, recon = codec.alloc(px * 2), codec.alloc(px * 2)
        coef = codec.alloc(px * 3)                                  # luma coefficients (2 B / px) or the CTU stream (3 B / px)
        res = codec.alloc(px * 3)                                   # the inverse batch's output on the unfused paths
        src, dst = codec.alloc(px * 3), codec.alloc(px * 3)        # the copy stream: up to 6 B / px of traffic
        for i, b in enumerate((pred, recon, coef, res, src)):
            codec.fill_residual_dev(b.ptr, b.nbytes // 2, 0x70 + i)
        codec.stream_sync()
        npl = px // 4
        calls = {
            "recon_luma_32": (4, lambda: codec.recon_luma_dev(pred.ptr, res.ptr, w, h, 32, recon.ptr)),
            "recon_luma_8": (4, lambda: codec.recon_luma_dev(pred.ptr, res.ptr, w, h, 8, recon.ptr)),
            "recon_chroma_8": (2, lambda: codec.recon_chroma_dev(pred.ptr, res.ptr, res.ptr + npl * 2, w, h, 8, recon.ptr)),
            "recon_chroma_32_pitch2": (2, lambda: codec.recon_chroma_dev(pred.ptr, res.ptr, res.ptr + 2048, w, h, 32, recon.ptr, 2)),
            "inv_to_tiles": (4, lambda: codec.dct32_inv_to_tiles_dev(coef.ptr, pred.ptr, w, h, recon.ptr)),
            "inv_then_recon (two calls)": (8, lambda: (codec.dct32_inv_dev(coef.ptr, res.ptr, n32),
                                                       codec.recon_luma_dev(pred.ptr, res.ptr, w, h, 32, recon.ptr))),
            "inv_ctu_to_tiles": (6, lambda: codec.dct32_inv_ctu_to_tiles_dev(coef.ptr, pred.ptr, w, h, recon.ptr)),
            "ctu unfused (inv + luma + chroma)": (12, lambda: (codec.dct32_inv_dev(coef.ptr, res.ptr, n_ctu * 6),
                                                               codec.recon_luma_dev(pred.ptr, res.ptr, w, h, 32, recon.ptr),
                                                               codec.recon_chroma_dev(pred.ptr, res.ptr + 8192, res.ptr + 10240, w, h, 32,
                                                                                      recon.ptr, 6))),
        }
        for bpp in sorted({b for b, _ in calls.values() if b <= 6}):
            calls["copy %d B/px" % bpp] = (bpp, lambda n=px * bpp // 2: codec.mem_ceiling_dev(0, src.ptr, dst.ptr, n))

        def timed(fn):
            codec.event_record(ev[0])
            for _ in range(REPS):
                fn()
            codec.event_record(ev[1])
            codec.stream_sync()
            return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

        for _, fn in calls.values():                                 # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        codec.stream_sync()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, (_, fn) in calls.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print("\n%d x %d (%d 32x32 luma blocks, %d CTUs), median of %d rounds x %d calls" % (w, h, n32, n_ctu, ROUNDS, REPS))
        print("%-36s %12s %9s %9s %9s %8s %8s" % ("call", "alg. bytes", "ms", "min ms", "TB/s", "of 8TB/s", "of copy"))
        for k, (bpp, _) in calls.items():
            nbytes = bpp * px
            tbs = nbytes / (med[k] * 1e-3) / 1e12
            copy = med.get("copy %d B/px" % bpp)
            frac = "%8.3f" % (copy / med[k]) if copy and not k.startswith("copy") else "%8s" % "-"
            print("%-36s %12d %9.4f %9.4f %9.3f %8.3f %s" % (k, nbytes, med[k], min(ms[k]), tbs, tbs / 8.0, frac))
        print("blocks/s, fused / two calls: luma %.2f x, whole CTU %.2f x" % (
            med["inv_then_recon (two calls)"] / med["inv_to_tiles"], med["ctu unfused (inv + luma + chroma)"] / med["inv_ctu_to_tiles"]))
        for b in (pred, recon, coef, res, src, dst):
            b.free()
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
