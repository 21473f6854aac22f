#!/usr/bin/env python3
"""Timing of inter prediction on tiled frames: the motion searches from tiles (xSatd8x8SearchFromTilesDev,
xSad8x8SearchFromTilesDev) against the planar searches on the same frame (the edge-padded plane), and integer-pel luma motion
compensation (xMotionCompLumaDev) against this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) over the bytes it moves --
device events after warm-up, all in ONE process, planar and tiled calls alternating within every round.
Usage: gpu_me_tiles.py [W H RANGE]  (default: 3840 2160 64).

MC moves 2.125 B per pixel: m_Y of the reference 1 (each output row is gathered once when the vectors are smooth), m_Y of the
prediction 1, one 8-byte record per 8x8 block 0.125.  A copy of B bytes moves 2 B, so the reference stream copies half of that;
"of copy" = copy time / call time."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
from bench_legs import smooth_frame_pair  # noqa: E402

ROUNDS, REPS = 9, 10


def main(argv):
    w, h, rng = (int(argv[0]), int(argv[1]), int(argv[2])) if argv else (3840, 2160, 64)
    assert w % 16 == 0 and h % 16 == 0
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    print("device: %s" % (codec.device_info(),))
    cur_h, refp_h = smooth_frame_pair(w, h, rng, 0x266)                     # planted motion (5, -3); refp_h is edge-padded by rng
    ref_h = np.ascontiguousarray(refp_h[rng:rng + h, rng:rng + w])
    refp_h = np.pad(ref_h, rng, mode="edge")                                 # the tiled calls' edge convention: both see the same samples
    nb = (w // 8) * (h // 8)
    d_cur, d_refp = codec.alloc(cur_h.nbytes), codec.alloc(refp_h.nbytes)
    d_cur.upload(cur_h)
    d_refp.upload(refp_h)
    rstride = refp_h.shape[1]
    origin = d_refp.ptr + rng * rstride + rng
    # the same frames as tiles, packed on the device (chroma: zeros)
    ct, rt = codec.alloc(w * h * 2), codec.alloc(w * h * 2)
    zc = codec.alloc(w * h // 4)
    zc.upload(np.zeros(w * h // 4, np.uint8))
    d_ref_plane = codec.alloc(ref_h.size)
    d_ref_plane.upload(ref_h)
    codec.conv_input_fmt_dev(ct.ptr, d_cur.ptr, zc.ptr, zc.ptr, w, w, h)
    codec.conv_input_fmt_dev(rt.ptr, d_ref_plane.ptr, zc.ptr, zc.ptr, w, w, h)
    best_p, best_t, pred = codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(w * h * 2)
    mc_bytes = w * h * 2 + nb * 8 + w * h // 8                                 # 2.125 B / px (see above)
    src, dst = codec.alloc(mc_bytes // 2 + 16), codec.alloc(mc_bytes // 2 + 16)
    codec.fill_residual_dev(src.ptr, (mc_bytes // 2 + 16) // 2, 0x71)
    codec.stream_sync()
    calls = {
        "satd planar": lambda: codec.satd_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr),
        "satd tiles": lambda: codec.satd_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr),
        "sad planar": lambda: codec.sad_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr),
        "sad tiles": lambda: codec.sad_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr),
        "mc luma": lambda: codec.motion_comp_luma_dev(rt.ptr, best_t.ptr, w, h, pred.ptr),
        "copy of the mc bytes": lambda: codec.mem_ceiling_dev(0, src.ptr, dst.ptr, (mc_bytes // 2) & ~15),
    }

    def timed(fn):
        codec.event_record(ev[0])
        for _ in range(REPS):
            fn()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in calls.values():                                           # warm-up: code objects, clocks, scratch
        for _ in range(3):
            fn()
    codec.stream_sync()
    # the records agree (the searches see the same samples)
    codec.satd_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr)
    codec.satd_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr)
    codec.stream_sync()
    assert np.array_equal(best_p.download(np.uint8, nb * 8), best_t.download(np.uint8, nb * 8))
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print("\n%d x %d, range +-%d (%d blocks), median of %d rounds x %d calls, planar and tiled alternating" % (w, h, rng, nb, ROUNDS, REPS))
    print("%-24s %9s %9s %9s %9s" % ("call", "ms", "min ms", "max ms", "spread"))
    for k in calls:
        print("%-24s %9.4f %9.4f %9.4f %8.1f%%" % (k, med[k], min(ms[k]), max(ms[k]), 100.0 * (max(ms[k]) - min(ms[k])) / med[k]))
    print("tiled / planar: SATD %.4f x, SAD %.4f x" % (med["satd tiles"] / med["satd planar"], med["sad tiles"] / med["sad planar"]))
    tbs = mc_bytes / (med["mc luma"] * 1e-3) / 1e12
    print("mc luma: %d bytes, %.2f us, %.3f TB/s, %.3f of the copy stream of the same bytes, %.2f %% of the tiled SATD search"
          % (mc_bytes, med["mc luma"] * 1e3, tbs, med["copy of the mc bytes"] / med["mc luma"], 100.0 * med["mc luma"] / med["satd tiles"]))
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
