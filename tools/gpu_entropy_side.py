#!/usr/bin/env python3
"""Timing and byte counts of the entropy coder of the side information (xEntropyEncodeSideGpu, xEntropyDecodeSideGpu) at 3840 x 2176, all
in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds.

The frame is the pair of tools/gpu_motion_pack.py (profiles/r28_motion_pack.txt) made 4:2:0 -- chroma is the luma plane's 2x2 means, U as
they are and V inverted --, predicted with the decided field of that tool, given a qp map by xAqStatsGpu / xAqDecideGpu (mode 2: offsets
against the frame's mean) and coded by
xDct32CodeMixedFrameGpu: kinds, modes, qp and coded flags are the chain's own.  Every region is 32x32 there, so a second coding of the
classes xTransformDecideCtuTilesGpu picks on the same frame is reported beside it.

  bytes         one frame's coded bytes of levels (xEntropyEncodeLevelsGpu), motion (xEntropyEncodeMvGpu) and side information; the CTUs
                that cost no side byte; the side bytes under the default table and under the frame's own best static table (per context
                the share of zero bins among the reference's bins, held to 31 .. 2017) -- found on the host, coded on the device
  device legs   (device events) encode count-only; encode with a stream of exactly the total; decode
  host leg      (host clock, from a synchronised device to the last byte on the host) the copy of the coded records and then of the coded
                words, beside the copy of the five dense arrays the stream replaces (d_kind, d_mode, d_class, d_qp, d_nnz)
  the decision  host/tdecide_example's frame (1920 x 1088, qp 32, lambda 368, all 13 candidates, its made-up class_bits): coded level bytes
                plus coded side bytes of xTransformDecideCtuTilesGpu against the all-32x32 xRdoQuantRegionsGpu chain

Everything is checked against tests/_entropy_side_ref.py before anything is timed.  No figure is a pass / fail condition, nothing is claimed
about bitrate beyond these bytes, and no table is tuned: the best static table is a measurement, not a default.
Usage: gpu_entropy_side.py [--out FILE] [--size W H]   (default profiles/r31_entropy_side.txt, 3840 2176)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402
import x266_amd.entropy as XE  # noqa: E402
import x266_amd.motion as XM  # noqa: E402
from gpu_aq import trimmed_mean  # noqa: E402
from gpu_motion_pack import decided_field  # noqa: E402

ROUNDS, REPS = 12, 10
QP, OFF, ROUNDING, PENALTY = 32, 0, 171, 64
ARRAYS = (("d_kind", np.uint8), ("d_mode", np.uint8), ("d_class", np.uint8), ("d_qp", np.uint8), ("d_nnz", np.uint32))


def coded_frame(codec, w, h):
    """(kinds, modes, qp bytes, nnz, levels, motion bytes, zero-byte motion CTUs) of the frame the docstring describes"""
    import _motion_ref as M
    import _tdecide_ref as T
    from _util import Oracle, me_frames
    oracle = Oracle()
    n_ctu = codec.ctu_count(w, h)
    cur, ref = me_frames(w, h, 0, 0x2121, mv=(11, -7))
    half = [(y.reshape(h // 2, 2, w // 2, 2).astype(np.uint32).sum((1, 3)) + 2 >> 2).astype(np.uint8) for y in (cur, ref)]
    tiles = [T.tiles_of_planes(oracle, y, c, 255 - c) for y, c in zip((cur, ref), half)]
    d_out, d_level, _ = decided_field(codec, w, h)
    nb = (w // 8) * (h // 8)
    field = d_out.download(np.uint8, 8 * nb).view(M.ME_DTYPE)
    mv = np.stack([field["mvx"], field["mvy"]], 1)
    pred = codec.motion_comp_qpel(tiles[1], mv, w, h)
    records, totals = codec.aq_stats(tiles[0], w, h)
    _, qps = codec.aq_decide(records, totals, w, h, mode=2, qp=QP, chroma_qp_offset=OFF)
    out = codec.code_mixed_frame(tiles[0], pred, w, h, qps=qps, qp=QP, rounding=ROUNDING, intra_penalty=PENALTY)
    ctu, words, _ = XM.motion_pack(codec, mv, d_level.download(np.uint8, nb), w, h)
    mcoded, _, _ = XE.entropy_encode_motion(codec, ctu, words, w, h)
    assert len(mcoded) == n_ctu
    return (out["kinds"].ravel(), out["modes"].ravel(), qps.ravel(), out["nnz"].ravel(), out["levels"].reshape(-1, 1024), int(mcoded["n_bytes"].sum()),
            int((mcoded["n_bytes"] == 0).sum()))


def best_static_table(S, ctus, qp, off):
    """per context the share of zero bins among the reference's bins of the frame, in 1/2048, held to 31 .. 2017"""
    zeros, ones = np.zeros(S.CONTEXTS), np.zeros(S.CONTEXTS)
    for ctu in ctus:
        for c, bit in S.ctu_bins(ctu, qp, off):
            if c is not None:
                (ones if bit else zeros)[c] += 1
    table = np.where(zeros + ones > 0, np.floor(2048.0 * zeros / np.maximum(zeros + ones, 1) + 0.5), 1024)
    return np.clip(table, 31, 2017).astype(np.uint16), zeros.astype(int), ones.astype(int)


def measure(codec, ev, w, h, say):
    import _entropy_side_ref as S
    n_ctu = codec.ctu_count(w, h)
    kind, mode, qps, nnz, levels, motion_bytes, motion_free = coded_frame(codec, w, h)
    lrec, _, _ = XE.entropy_encode_levels(codec, levels, None, nnz)
    level_bytes = int(lrec["n_bytes"].sum())
    arrays = dict(d_kind=kind, d_mode=mode, d_qp=qps, d_nnz=nnz)
    al = codec.alloc
    d_in = {name: codec._upload(np.ascontiguousarray(a)) for name, a in arrays.items()}
    d_coded, d_total, d_status = al(32 * n_ctu), al(16), al(max(n_ctu, 16))
    d_back = {name: al(6 * n_ctu * np.dtype(dt).itemsize) for name, dt in ARRAYS}
    ptrs = {name: d.ptr for name, d in d_in.items()}
    enc0 = XE.entropy_side_params(d_coded=d_coded.ptr, d_total=d_total.ptr, n_ctu=n_ctu, qp=QP, chroma_qp_offset=OFF, **ptrs)
    XE.entropy_encode_side_dev(codec, enc0)
    codec.stream_sync()
    coded_words = int(d_total.download(np.uint64, 2)[0])
    d_stream = al(2 * coded_words + 16)
    enc = XE.entropy_side_params(d_coded=d_coded.ptr, d_stream=d_stream.ptr, d_total=d_total.ptr, n_ctu=n_ctu, cap_words=coded_words, qp=QP, chroma_qp_offset=OFF, **ptrs)
    dec = XE.entropy_side_params(d_coded=d_coded.ptr, d_stream=d_stream.ptr, d_status=d_status.ptr, n_ctu=n_ctu, cap_words=coded_words, qp=QP, chroma_qp_offset=OFF,
                                 **{name: d.ptr for name, d in d_back.items()})

    # one pass, checked against the reference
    XE.entropy_encode_side_dev(codec, enc)
    XE.entropy_decode_side_dev(codec, dec)
    codec.stream_sync()
    coded, stream = d_coded.download(np.uint8, 32 * n_ctu).view(S.CODED_DTYPE), d_stream.download(np.uint16, coded_words)
    want, want_stream, want_total = S.encode(n_ctu, kind, mode, None, qps, nnz, qp=QP, off=OFF)
    assert np.array_equal(coded, want) and np.array_equal(stream, want_stream) and int(want_total[0]) == coded_words, "encode differs from the reference"
    ctus = S.canon_arrays(n_ctu, kind, mode, None, qps, nnz, QP, OFF)
    back = {name: d_back[name].download(dt, 6 * n_ctu) for name, dt in ARRAYS}
    for i, name in ((0, "d_kind"), (1, "d_mode"), (3, "d_class"), (4, "d_qp"), (2, "d_nnz")):
        assert np.array_equal(back[name], np.array([v for ctu in ctus for v in ctu[i]], back[name].dtype)), "decode does not return the canonical " + name
    assert not d_status.download(np.uint8, n_ctu).any()
    side_bytes = int(coded["n_bytes"].sum())
    table, zeros, ones = best_static_table(S, ctus, QP, OFF)
    best, _, _ = XE.entropy_encode_side(codec, n_ctu, kind, mode, None, qps, nnz, qp=QP, chroma_qp_offset=OFF, init=table)
    assert np.array_equal(best, S.encode(n_ctu, kind, mode, None, qps, nnz, qp=QP, off=OFF, init=table)[0])
    say("\n%d x %d: %d CTUs, %d regions; qp %d under the map of xAqDecideGpu, mode 2 (region qp %d .. %d), %d intra regions, %d coded regions"
        % (w, h, n_ctu, 6 * n_ctu, QP, int(qps.min()), int(qps.max()), int(coded["n_intra"].sum()), int(coded["n_coded"].sum())))
    say("coded records, stream and totals equal tests/_entropy_side_ref.py's; decode returns the canonical form of the input")
    say("one frame's coded bytes: levels %d, motion %d, side %d  (side / motion %.2f, side / levels %.4f)"
        % (level_bytes, motion_bytes, side_bytes, side_bytes / max(1, motion_bytes), side_bytes / max(1, level_bytes)))
    say("CTUs that cost no side byte: %d of %d (no motion byte: %d); the longest side substream %d bytes; %d context and %d bypass bins in all, %.2f bins per coded bit"
        % (int((coded["n_bytes"] == 0).sum()), n_ctu, motion_free, int(coded["n_bytes"].max()), int(coded["ctx_bins"].sum()), int(coded["bypass_bins"].sum()),
           (int(coded["ctx_bins"].sum()) + int(coded["bypass_bins"].sum())) / max(1, 8 * side_bytes)))
    say("side bytes under the default table %d, under the frame's own best static table %d (%.3f); that table: %s"
        % (side_bytes, int(best["n_bytes"].sum()), int(best["n_bytes"].sum()) / max(1, side_bytes), " ".join(str(int(x)) for x in table)))
    say("zero / one bins per context: " + " ".join("%d/%d" % (z, o) for z, o in zip(zeros, ones)))
    dense_bytes = 48 * n_ctu
    say("the five dense arrays are %d bytes (48 per CTU); coded records + words %d bytes (%d + %d)" % (dense_bytes, 32 * n_ctu + 2 * coded_words, 32 * n_ctu, 2 * coded_words))

    calls = {"encode, count-only": lambda: XE.entropy_encode_side_dev(codec, enc0), "encode": lambda: XE.entropy_encode_side_dev(codec, enc),
             "decode": lambda: XE.entropy_decode_side_dev(codec, dec)}

    def timed(k):
        codec.event_record(ev[0])
        for _ in range(REPS):
            calls[k]()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    host = dict(coded=np.ones(32 * n_ctu, np.uint8), stream=np.ones(max(coded_words, 1), np.uint16))
    host.update({name: np.ones(6 * n_ctu, dt) for name, dt in ARRAYS})

    def copy(name, src, nbytes):
        if nbytes:
            codec._check(codec.L.xHipMemcpyD2H(codec.ctx, host[name].ctypes.data, src.ptr, nbytes), "xHipMemcpyD2H")

    def dense_copy():
        for name, dt in ARRAYS:
            copy(name, d_back[name], 6 * n_ctu * np.dtype(dt).itemsize)

    def coded_copy():
        copy("coded", d_coded, 32 * n_ctu)
        last = host["coded"].view(S.CODED_DTYPE)[-1]
        copy("stream", d_stream, 2 * (int(last["offset"]) + int(last["n_words"])))

    hosts = {"host: the five dense arrays": dense_copy, "host: coded records + words": coded_copy}

    def host_timed(k):
        codec.stream_sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            hosts[k]()
        return (time.perf_counter() - t0) * 1e3 / REPS

    for fn in list(calls.values()) + list(hosts.values()):               # warm-up: code objects, clocks, the copy paths
        for _ in range(2):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in list(calls) + list(hosts)}
    for _ in range(ROUNDS):
        for k in calls:
            ms[k].append(timed(k))
        for k in hosts:
            ms[k].append(host_timed(k))
    assert np.array_equal(host["coded"].view(S.CODED_DTYPE), want) and np.array_equal(host["stream"][:coded_words], want_stream)
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    say("10 %% trimmed mean of %d rounds of %d back-to-back repetitions, all legs alternating; device legs by device events, host legs by the host's clock" % (ROUNDS, REPS))
    say("%-32s %10s %10s %10s" % ("leg", "us", "min us", "max us"))
    for k in ms:
        say("%-32s %10.1f %10.1f %10.1f" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3))
    say("count-only / encode = %.2f; coded copy / dense copy = %.3f; encode + coded copy against the dense copy %.2f"
        % (t["encode, count-only"] / t["encode"], t["host: coded records + words"] / t["host: the five dense arrays"],
           (t["encode"] + t["host: coded records + words"]) / t["host: the five dense arrays"]))
    say("the motion coder at the same CTU count, one wave per CTU: tools/gpu_entropy_motion.py, run in the same session on the same box (below)")


def tdecide_example_frames(w, h):
    """the planes of host/tdecide_example.c: (cur, ref), each (y, u, v)"""
    def hash2(a, b):
        x = (a.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (b.astype(np.uint32) * np.uint32(0x85EBCA77))
        x ^= x >> np.uint32(15)
        x = x * np.uint32(0x2C1B3C6D)
        return x ^ (x >> np.uint32(13))

    def plane(p, frame):
        ph, pw = (h // 2, w // 2) if p else (h, w)
        yy, xx = np.mgrid[0:ph, 0:pw].astype(np.int64)
        x, y = (2 * xx, 2 * yy) if p else (xx, yy)
        u, v = x + (0 if frame else 3), y + (0 if frame else -2)
        val = 128 + np.floor(80.0 * (((u * 5 + v * 3 + 17 * p) % 193) / 193.0)).astype(np.int64) - 40
        if frame:
            cell = 32 if p else 64
            kind = hash2(x // cell, y // cell + 977 * p) & np.uint32(3)
            r = hash2(x + 4099 * p, y).astype(np.int64)
            val = val + np.where(kind == 1, r % 13 - 6, 0) + np.where(kind == 2, np.where(r % 211 == 0, 70, r % 3 - 1), 0) + np.where(kind == 3, ((x + y) % 8) * 4 - 14, 0)
        return np.clip(val, 0, 255).astype(np.uint8)

    return [plane(p, 1) for p in range(3)], [plane(p, 0) for p in range(3)]


def decision_ratio(codec, say, w=1920, h=1088, qp=32, lam=368):
    import _entropy_side_ref as S
    import _tdecide_ref as T
    from _util import Oracle
    oracle = Oracle()
    cur, ref = tdecide_example_frames(w, h)
    n_ctu, nb = codec.ctu_count(w, h), (w // 8) * (h // 8)
    cur_t, ref_t = T.tiles_of_planes(oracle, *cur), T.tiles_of_planes(oracle, *ref)
    d_cur, d_ref, d_int, d_q = codec._upload(cur_t), codec._upload(ref_t), codec.alloc(8 * nb), codec.alloc(8 * nb)
    codec.satd_search_from_tiles_dev(d_cur.ptr, d_ref.ptr, w, h, 8, d_int.ptr)
    codec.satd_refine_qpel_from_tiles_dev(d_cur.ptr, d_ref.ptr, w, h, d_int.ptr, d_q.ptr)
    codec.stream_sync()
    mv = d_q.download(np.int16, 4 * nb).reshape(nb, 4)[:, :2]
    pred = codec.motion_comp_qpel(ref_t, mv, w, h)
    class_bits = [16 * (1 + (3 - (k & 3)) + (2 if k >> 2 else 1)) for k in range(16)]
    cls, lv, nnz, stat, _ = codec.transform_decide(cur_t, pred, w, h, qp=qp, lam=lam, class_bits=class_bits)
    coef = codec.transform_ctu_from_tiles(cur_t, pred, w, h, np.full(6 * n_ctu, 3, np.uint8)).reshape(-1, 1024)
    lv32, nnz32, stat32 = codec.rdo_quant(coef, None, None, qp, lam)
    rows = {}
    for name, levels, classes, counts, records in (("decided", lv, cls, nnz, stat), ("all 32x32", lv32, None, nnz32, stat32)):
        lrec, _, _ = XE.entropy_encode_levels(codec, levels, classes, counts)
        srec, _, _ = XE.entropy_encode_side(codec, n_ctu, None, None, classes, None, counts, qp=qp)
        assert np.array_equal(srec, S.encode(n_ctu, None, None, classes, None, counts, qp=qp)[0])
        rows[name] = (int(records["bits"].astype(np.int64).sum()), int(lrec["n_bytes"].sum()), int(srec["n_bytes"].sum()))
    say("\nhost/tdecide_example's frame, %d x %d, qp %d, lambda %d, all 13 candidates, its made-up class_bits; side = kinds (all inter), coded flags, classes, qp (no difference)"
        % (w, h, qp, lam))
    say("%-10s %20s %18s %18s %18s" % ("", "estimated bits (q4)", "coded level bytes", "coded side bytes", "level + side"))
    for name, (bits, lb, sb) in rows.items():
        say("%-10s %20d %18d %18d %18d" % (name, bits, lb, sb, lb + sb))
    d, a = rows["decided"], rows["all 32x32"]
    say("decided / all 32x32: estimated bits %.3f, coded level bytes %.3f, coded level + side bytes %.3f; the classes of the decided frame: %s"
        % (d[0] / a[0], d[1] / a[1], (d[1] + d[2]) / (a[1] + a[2]), ", ".join("%d: %d" % (k, c) for k, c in enumerate(np.bincount(cls, minlength=16)) if c)))


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "r31_entropy_side.txt")
    size = (3840, 2176)
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    if "--size" in argv:
        size = (int(argv[argv.index("--size") + 1]), int(argv[argv.index("--size") + 2]))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    say("device: %s" % (codec.device_info(),))
    measure(codec, ev, size[0], size[1], say)
    decision_ratio(codec, say)
    for e in ev:
        codec.event_destroy(e)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
