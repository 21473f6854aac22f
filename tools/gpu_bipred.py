#!/usr/bin/env python3
"""Timing of bi-directional inter prediction on one frame (default 3840 x 2176: the calls take multiples of 16), device events after
warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  bi mc luma / chroma / fused     xMotionCompBiQpelTiles, planes 1 / 2 / 3, every block of direction 3, default weights
  bi mc fused, weighted           the same with an x266_wp_t
  two uni mc fused                xMotionCompQpelGpu twice, list 0 and list 1 (what a host-side average would start from)
  bi costs                        xSatd8x8BiCostsFromTiles, costs and directions
  bi refine / uni refine          xSatd8x8RefineBiQpelFromTiles next to xSatd8x8RefineQpelFromTilesGpu, both without a cost map

Ratios: bi mc fused / two uni mc fused, bi refine / uni refine.  No rate is a pass / fail condition.
The frames are a sinusoid with noise, list 0 and list 1 moved copies of it; the vectors are small quarter-sample vectors of every
phase.  Before timing, the fused call is held against the two single-plane calls, and directions 1 and 2 against the uni call.
Usage: gpu_bipred.py [W H] [--out FILE]   (default profiles/r16_bipred.txt: the measured part; the resource report and the
reading below it in the committed file are appended by hand)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS = 20, 20


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def frame(rs, w, h, dx, dy):
    yy, xx = np.mgrid[0:h, 0:w]
    plane = lambda ph, pw, s: np.clip(128 + (70 * np.sin((xx[:ph, :pw] * s + dx) / 9.0) * np.cos((yy[:ph, :pw] * s + dy) / 13.0)).astype(np.int64)
                                      + rs.randint(-6, 7, (ph, pw)), 0, 255).astype(np.uint8)
    y, u, v = plane(h, w, 1), plane(h // 2, w // 2, 2), plane(h // 2, w // 2, 2)
    t = rs.randint(0, 256, (h // 16, w // 16, 512)).astype(np.uint8)
    t[:, :, :256] = y.reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)
    t[:, :, 256:384] = np.stack([u, v], axis=-1).reshape(h // 16, 8, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 128)
    return t.ravel()


def records(mv):
    rec = np.zeros((len(mv), 4), np.int16)
    rec[:, :2] = mv
    return rec


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r16_bipred.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    w, h = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3840, 2176)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    nb, nt, tile_bytes = (w // 8) * (h // 8), (w // 16) * (h // 16), w * h * 2
    rs = np.random.RandomState(0x266)

    def up(a):
        d = codec.alloc(max(a.nbytes, 16))
        d.upload(np.ascontiguousarray(a))
        return d

    cur, ref0, ref1 = up(frame(rs, w, h, 0, 0)), up(frame(rs, w, h, 2.25, -1.5)), up(frame(rs, w, h, -1.75, 0.5))
    m_int = rs.randint(-3, 4, (nb, 2)).astype(np.int16)
    mv0, mv1 = (4 * m_int + rs.randint(-3, 4, (nb, 2))).astype(np.int16), rs.randint(-15, 16, (nb, 2)).astype(np.int16)
    d_mv0, d_mv1, d_int = up(records(mv0)), up(records(mv1)), up(records(m_int))
    pred, pred2, pred3 = (codec.alloc(tile_bytes) for _ in range(3))
    costs, dirs, best = codec.alloc(nb * 12), codec.alloc(nb), codec.alloc(nb * 8)
    wp = codec.wp_params(w=((40, 36, 36), (24, 28, 28)), o=((2, 0, 0), (-1, 0, 0)), log2_denom=(5, 5))

    # the fused call is the pair, directions 1 and 2 are the uni call (on this frame; the tests hold the statement)
    zero = np.zeros(tile_bytes, np.uint8)
    for p in (pred, pred2, pred3):
        p.upload(zero)
    codec.motion_comp_bi_qpel_dev(ref0.ptr, ref1.ptr, d_mv0.ptr, d_mv1.ptr, w, h, pred.ptr, planes=3)
    codec.motion_comp_bi_qpel_dev(ref0.ptr, ref1.ptr, d_mv0.ptr, d_mv1.ptr, w, h, pred2.ptr, planes=1)
    codec.motion_comp_bi_qpel_dev(ref0.ptr, ref1.ptr, d_mv0.ptr, d_mv1.ptr, w, h, pred2.ptr, planes=2)
    codec.stream_sync()
    assert np.array_equal(pred.download(np.uint8, tile_bytes), pred2.download(np.uint8, tile_bytes)), "the fused call differs from the pair"
    for d, (r, m) in ((1, (ref0, d_mv0)), (2, (ref1, d_mv1))):
        dd = up(np.full(nb, d, np.uint8))
        codec.motion_comp_bi_qpel_dev(ref0.ptr, ref1.ptr, d_mv0.ptr, d_mv1.ptr, w, h, pred2.ptr, dd.ptr)
        codec.motion_comp_qpel_dev(r.ptr, m.ptr, w, h, pred3.ptr)
        codec.stream_sync()
        assert np.array_equal(pred2.download(np.uint8, tile_bytes), pred3.download(np.uint8, tile_bytes)), "direction %d differs from the uni call" % d
    codec.satd8x8_bi_costs_dev(cur.ptr, ref0.ptr, ref1.ptr, w, h, d_mv0.ptr, d_mv1.ptr, costs.ptr, dirs.ptr, bi_penalty=16)
    codec.stream_sync()
    say("\n%d x %d (%d tiles, %d blocks): directions 1 / 2 / 3 with penalty 16: %s" % (
        w, h, nt, nb, np.bincount(dirs.download(np.uint8, nb), minlength=4)[1:4].tolist()))

    def two_uni():
        codec.motion_comp_qpel_dev(ref0.ptr, d_mv0.ptr, w, h, pred2.ptr)
        codec.motion_comp_qpel_dev(ref1.ptr, d_mv1.ptr, w, h, pred3.ptr)

    bi = lambda planes, weights=None: codec.motion_comp_bi_qpel_dev(ref0.ptr, ref1.ptr, d_mv0.ptr, d_mv1.ptr, w, h, pred.ptr, 0, weights, planes)
    # bytes a call reads plus writes once (vectors and small outputs included)
    calls = {"bi mc luma": (lambda: bi(1), nt * 768 + nb * 16), "bi mc chroma": (lambda: bi(2), nt * 384 + nb * 16),
             "bi mc fused": (lambda: bi(3), nt * 1152 + nb * 16), "bi mc fused, weighted": (lambda: bi(3, wp), nt * 1152 + nb * 16),
             "two uni mc fused": (two_uni, nt * 1536 + nb * 16),
             "bi costs": (lambda: codec.satd8x8_bi_costs_dev(cur.ptr, ref0.ptr, ref1.ptr, w, h, d_mv0.ptr, d_mv1.ptr, costs.ptr, dirs.ptr, bi_penalty=16),
                          nt * 768 + nb * 29),
             "bi refine": (lambda: codec.satd8x8_refine_bi_qpel_dev(cur.ptr, ref1.ptr, d_mv1.ptr, ref0.ptr, d_int.ptr, 0, w, h, best.ptr), nt * 768 + nb * 24),
             "uni refine": (lambda: codec.satd_refine_qpel_from_tiles_dev(cur.ptr, ref0.ptr, w, h, d_int.ptr, best.ptr), nt * 512 + nb * 16)}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k][0]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn, _ in calls.values():                                        # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d calls, all legs alternating" % (ROUNDS, REPS))
    say("%-24s %9s %9s %9s %9s" % ("leg", "us", "min us", "max us", "GB/s"))
    for k in calls:
        say("%-24s %9.2f %9.2f %9.2f %9.0f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, calls[k][1] / t[k] / 1e6))
    say("bi mc fused / two uni mc fused %.3f" % (t["bi mc fused"] / t["two uni mc fused"]))
    say("bi refine / uni refine %.3f" % (t["bi refine"] / t["uni refine"]))
    say("bi mc fused / (bi mc luma + bi mc chroma) %.3f" % (t["bi mc fused"] / (t["bi mc luma"] + t["bi mc chroma"])))
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
