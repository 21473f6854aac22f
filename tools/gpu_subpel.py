#!/usr/bin/env python3
"""Timing of quarter-sample prediction on a 4K frame (3840 x 2160), device events after warm-up, all in ONE process, the legs
alternating within every round, 10 % trimmed mean over the rounds:

  int luma / chroma / fused     xMotionCompLumaDev / ChromaDev / Dev on the searched integer vectors m
  4m  luma / chroma / fused     xMotionCompQpelLumaGpu / ChromaGpu / Gpu on the vectors 4 m (the same bytes as the integer calls)
  ref luma / chroma / fused     the same three calls on the refined vectors
  search                        xSatd8x8SearchFromTilesDev at range 16
  refine, refine + costs        xSatd8x8RefineQpelFromTilesGpu without and with d_costs

The motion compensation legs stand next to this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) of the bytes a call reads
once and writes once (luma 256 + 256, chroma 128 + 128, fused 384 + 384 per tile, plus a record per block); "of copy" = copy
time / call time.  The refinement stands next to the search.  Ratios a reviewer asks for: fused / (luma + chroma back to back),
and quarter-sample on 4 m / integer call.
Usage: gpu_subpel.py [W H]   (default 3840 2160)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS, SEARCH_REPS, RANGE = 20, 50, 5, 16


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def smooth_frame(rs, w, h):
    """a tile array whose luma is low-passed noise (so that the search finds motion), chroma and m_I random"""
    y = rs.randint(0, 256, (h + 8, w + 8)).astype(np.float64)
    k = np.ones(5) / 5.0
    y = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, y)
    y = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, y)
    return np.clip((y - 128.0) * 3.0 + 128.0, 0, 255).astype(np.uint8)


def tiles_of(y, rs):
    h, w = y.shape
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    return t.ravel()


def main(argv):
    w, h = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3840, 2160)
    assert w % 16 == 0 and h % 16 == 0
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    print("device: %s" % (codec.device_info(),))
    nb, nt, tile_bytes = (w // 8) * (h // 8), (w // 16) * (h // 16), w * h * 2
    rs = np.random.RandomState(0x266)
    big = smooth_frame(rs, w, h)
    cur_h = tiles_of(big[4:4 + h, 4:4 + w], rs)
    ref_h = tiles_of(np.clip(big[2:2 + h, 7:7 + w].astype(np.int16) + rs.randint(-5, 6, (h, w)), 0, 255).astype(np.uint8), rs)
    cur, ref, pred = codec.alloc(tile_bytes), codec.alloc(tile_bytes), codec.alloc(tile_bytes)
    cur.upload(cur_h)
    ref.upload(ref_h)
    d_int, d_4m, d_ref, d_costs = codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(nb * 8), codec.alloc(nb * 196)
    codec.satd_search_from_tiles_dev(cur.ptr, ref.ptr, w, h, RANGE, d_int.ptr)
    codec.satd_refine_qpel_from_tiles_dev(cur.ptr, ref.ptr, w, h, d_int.ptr, d_ref.ptr)
    codec.stream_sync()
    rec = d_int.download(np.uint8, nb * 8).view(np.int16).reshape(nb, 4).copy()
    rec[:, :2] *= 4
    d_4m.upload(rec)
    q = d_ref.download(np.uint8, nb * 8).view(np.int16).reshape(nb, 4)[:, :2]
    print("refined vectors: %.1f %% of the blocks moved off the integer position, %.1f %% have a 2-D luma phase"
          % (100.0 * (q != rec[:, :2]).any(axis=1).mean(), 100.0 * ((q & 3) != 0).all(axis=1).mean()))
    # 4 m reproduces the integer calls
    codec.motion_comp_dev(ref.ptr, d_int.ptr, w, h, pred.ptr)
    codec.stream_sync()
    want = pred.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384].copy()
    codec.motion_comp_qpel_dev(ref.ptr, d_4m.ptr, w, h, pred.ptr)
    codec.stream_sync()
    assert np.array_equal(pred.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384], want), "4 m differs from the integer calls"

    planes = {"luma": 512, "chroma": 256, "fused": 768}                 # bytes read once + written once per tile
    int_calls = {"luma": codec.motion_comp_luma_dev, "chroma": codec.motion_comp_chroma_dev, "fused": codec.motion_comp_dev}
    q_calls = {"luma": codec.motion_comp_qpel_luma_dev, "chroma": codec.motion_comp_qpel_chroma_dev, "fused": codec.motion_comp_qpel_dev}
    calls, reps = {}, {}
    for p in planes:
        calls["int " + p] = lambda p=p: int_calls[p](ref.ptr, d_int.ptr, w, h, pred.ptr)
        calls["4m  " + p] = lambda p=p: q_calls[p](ref.ptr, d_4m.ptr, w, h, pred.ptr)
        calls["ref " + p] = lambda p=p: q_calls[p](ref.ptr, d_ref.ptr, w, h, pred.ptr)
    half = (nt * 768 + nb * 8) // 2
    src, dst = codec.alloc(half), codec.alloc(half)
    codec.fill_residual_dev(src.ptr, half // 2, 0x71)
    for p, per_tile in planes.items():
        calls["copy of the %s bytes" % p] = lambda n=(nt * per_tile + nb * 8) // 2: codec.mem_ceiling_dev(0, src.ptr, dst.ptr, n & ~15)
    calls["search"] = lambda: codec.satd_search_from_tiles_dev(cur.ptr, ref.ptr, w, h, RANGE, d_int.ptr)
    calls["refine"] = lambda: codec.satd_refine_qpel_from_tiles_dev(cur.ptr, ref.ptr, w, h, d_int.ptr, d_ref.ptr)
    calls["refine + costs"] = lambda: codec.satd_refine_qpel_from_tiles_dev(cur.ptr, ref.ptr, w, h, d_int.ptr, d_ref.ptr, d_costs.ptr)
    for k in calls:
        reps[k] = SEARCH_REPS if k == "search" else REPS

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(reps[k]):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / reps[k]

    for fn in calls.values():                                           # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    print("\n%d x %d (%d tiles, %d blocks): 10 %% trimmed mean of %d rounds, all legs alternating" % (w, h, nt, nb, ROUNDS))
    print("%-26s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "of copy"))
    for k in calls:
        of = "%9.3f" % (t["copy of the %s bytes" % k[4:]] / t[k]) if k[:4] in ("int ", "4m  ", "ref ") else ""
        print("%-26s %9.2f %9.2f %9.2f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, of))
    for kind in ("4m  ", "ref "):
        print("%s: fused / (luma + chroma back to back) %.3f" % (kind.strip(), t[kind + "fused"] / (t[kind + "luma"] + t[kind + "chroma"])))
    for p in planes:
        print("%-6s: quarter-sample on 4 m / integer call %.3f" % (p, t["4m  " + p] / t["int " + p]))
    print("refine / search at range %d: %.3f; with d_costs %.3f" % (RANGE, t["refine"] / t["search"], t["refine + costs"] / t["search"]))
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
