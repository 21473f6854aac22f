#!/usr/bin/env python3
"""Timing of inter prediction on tiled frames: the motion searches from tiles (xSatd8x8SearchFromTilesDev,
xSad8x8SearchFromTilesDev) against the planar searches on the same frame (the edge-padded plane), and motion compensation on
the searched vectors -- luma (xMotionCompLumaDev), chroma (xMotionCompChromaDev), both in one launch (xMotionCompDev) and the
two single calls back to back -- each against this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) over the bytes it
moves: device events after warm-up, all in ONE process, the calls alternating within every round.
Usage: gpu_me_tiles.py [W H RANGE] [--ref-lib PATH]  (default: 3840 2160 64).  --ref-lib: another revision's library
(tools/ab_build.sh <git-ref> -> tools/_ab/libx266hip_ref.so) whose xMotionCompLumaDev joins the rounds as "mc luma (ref lib)".

Luma MC moves 2.125 B per pixel: m_Y of the reference 1 (each output row is gathered once when the vectors are smooth), m_Y of
the prediction 1, one 8-byte record per 8x8 block 0.125; chroma MC 1.125 (m_C is 0.5 B per pixel each way), both 3.125 (the
records once).  A copy of B bytes moves 2 B, so the reference stream copies half of that; "of copy" = copy time / call time."""
import ctypes
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
MC_REPS = 100                                                            # calls of microseconds: a longer window per round


def ref_lib_luma(path):
    """xMotionCompLumaDev of another build of the library, on a context of its own (same process, same buffers, null stream)"""
    P = ctypes.c_void_p
    L = ctypes.CDLL(path)
    ctx = P()
    assert L.xHipCodecInit(ctypes.byref(ctx), 0) == 0
    L.xMotionCompLumaDev.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, P, P]
    return lambda ref, mv, w, h, pred: L.xMotionCompLumaDev(ctx, ref, mv, w, h, pred, None)


def main(argv):
    ref_lib = None
    if "--ref-lib" in argv:
        k = argv.index("--ref-lib")
        ref_lib, argv = argv[k + 1], argv[:k] + argv[k + 2:]
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
    # the same frames as tiles, packed on the device (chroma: the luma planes subsampled, so that the filter sees a picture)
    ct, rt = codec.alloc(w * h * 2), codec.alloc(w * h * 2)
    d_ref_plane = codec.alloc(ref_h.size)
    d_ref_plane.upload(ref_h)
    chroma = []
    for plane in (cur_h, ref_h):
        cu, cv = codec.alloc(w * h // 4), codec.alloc(w * h // 4)
        cu.upload(np.ascontiguousarray(plane[::2, ::2]))
        cv.upload(np.ascontiguousarray(plane[1::2, 1::2]))
        chroma.append((cu, cv))
    codec.conv_input_fmt_dev(ct.ptr, d_cur.ptr, chroma[0][0].ptr, chroma[0][1].ptr, w, w, h)
    codec.conv_input_fmt_dev(rt.ptr, d_ref_plane.ptr, chroma[1][0].ptr, chroma[1][1].ptr, w, w, h)
    best_p, best_t, pred = codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(w * h * 2)
    mc_bytes = {"mc luma": w * h * 2 + nb * 8, "mc chroma": w * h + nb * 8, "mc both": w * h * 3 + nb * 8}   # 2.125 / 1.125 / 3.125 B / px
    src, dst = codec.alloc(mc_bytes["mc both"] // 2 + 16), codec.alloc(mc_bytes["mc both"] // 2 + 16)
    codec.fill_residual_dev(src.ptr, (mc_bytes["mc both"] // 2 + 16) // 2, 0x71)
    codec.stream_sync()
    calls = {
        "satd planar": lambda: codec.satd_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr),
        "satd tiles": lambda: codec.satd_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr),
        "sad planar": lambda: codec.sad_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr),
        "sad tiles": lambda: codec.sad_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr),
        "mc luma": lambda: codec.motion_comp_luma_dev(rt.ptr, best_t.ptr, w, h, pred.ptr),
        "mc chroma": lambda: codec.motion_comp_chroma_dev(rt.ptr, best_t.ptr, w, h, pred.ptr),
        "mc both": lambda: codec.motion_comp_dev(rt.ptr, best_t.ptr, w, h, pred.ptr),
        "mc luma + mc chroma": lambda: (codec.motion_comp_luma_dev(rt.ptr, best_t.ptr, w, h, pred.ptr),
                                        codec.motion_comp_chroma_dev(rt.ptr, best_t.ptr, w, h, pred.ptr)),
    }
    if ref_lib:
        ref_luma = ref_lib_luma(ref_lib)
        calls["mc luma (ref lib)"] = lambda: ref_luma(rt.ptr, best_t.ptr, w, h, pred.ptr)
    for k, nbytes in mc_bytes.items():
        calls["copy of the %s bytes" % k] = lambda nbytes=nbytes: codec.mem_ceiling_dev(0, src.ptr, dst.ptr, (nbytes // 2) & ~15)

    def timed(fn, reps):
        codec.event_record(ev[0])
        for _ in range(reps):
            fn()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / reps

    for fn in calls.values():                                           # warm-up: code objects, clocks, scratch
        for _ in range(3):
            fn()
    codec.stream_sync()
    # the records agree (the searches see the same samples)
    codec.satd_search_dev(d_cur.ptr, w, origin, rstride, w, h, rng, best_p.ptr)
    codec.satd_search_from_tiles_dev(ct.ptr, rt.ptr, w, h, rng, best_t.ptr)
    codec.stream_sync()
    assert np.array_equal(best_p.download(np.uint8, nb * 8), best_t.download(np.uint8, nb * 8))
    # the fused call writes the bytes of the two single calls (pred is rewritten by every leg)
    calls["mc luma + mc chroma"]()
    codec.stream_sync()
    two = pred.download(np.uint8, w * h * 2)
    codec.fill_residual_dev(pred.ptr, w * h, 0x72)
    calls["mc both"]()
    codec.stream_sync()
    one = pred.download(np.uint8, w * h * 2).reshape(-1, 512)
    assert np.array_equal(one[:, :384], two.reshape(-1, 512)[:, :384])
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn, MC_REPS if ("mc " in k) else REPS))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print("\n%d x %d, range +-%d (%d blocks), median of %d rounds x %d calls (searches) / %d calls (mc and copy legs), all legs alternating"
          % (w, h, rng, nb, ROUNDS, REPS, MC_REPS))
    print("%-28s %9s %9s %9s %9s" % ("call", "ms", "min ms", "max ms", "spread"))
    for k in calls:
        print("%-28s %9.4f %9.4f %9.4f %8.1f%%" % (k, med[k], min(ms[k]), max(ms[k]), 100.0 * (max(ms[k]) - min(ms[k])) / med[k]))
    print("tiled / planar: SATD %.4f x, SAD %.4f x" % (med["satd tiles"] / med["satd planar"], med["sad tiles"] / med["sad planar"]))
    spread = lambda k: max(ms[k]) - min(ms[k])
    for k, nbytes in mc_bytes.items():
        print("%s: %d bytes, %.2f us, %.3f TB/s, %.3f of the copy stream of the same bytes, %.2f %% of the tiled SATD search"
              % (k, nbytes, med[k] * 1e3, nbytes / (med[k] * 1e-3) / 1e12, med["copy of the %s bytes" % k] / med[k], 100.0 * med[k] / med["satd tiles"]))
    two, one = "mc luma + mc chroma", "mc both"
    print("mc both - (mc luma + mc chroma back to back): %+.2f us (spreads %.2f / %.2f us): the fused call %s"
          % ((med[one] - med[two]) * 1e3, spread(one) * 1e3, spread(two) * 1e3,
             "is no slower" if med[one] <= med[two] + max(spread(one), spread(two)) else "IS SLOWER"))
    if ref_lib:
        new, old = "mc luma", "mc luma (ref lib)"
        print("mc luma - mc luma (ref lib): %+.2f us (spreads %.2f / %.2f us): %s"
              % ((med[new] - med[old]) * 1e3, spread(new) * 1e3, spread(old) * 1e3,
                 "no slower" if med[new] <= med[old] + max(spread(new), spread(old)) else "SLOWER"))
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
