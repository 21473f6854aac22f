#!/usr/bin/env python3
"""Timing of the quantiser and of the fused CTU coding call on a 4K frame (3840 x 2176, a multiple of 64), device events after
warm-up, all in ONE process, the legs alternating within every round, 10 % trimmed mean over the rounds:

  regions     xQuantRegionsGpu(0) over the frame's 12 KiB-per-CTU stream, out of place          4 KiB per region
  fused       xDct32CodeCtuTilesGpu (levels, non-zero counts, reconstruction over pred)         30 KiB per CTU
  chain       xDct32FwdCtuFromTilesDev -> xQuantRegionsGpu(0) -> xQuantRegionsGpu(1) -> xDct32InvCtuToTilesDev, in place   96 KiB per CTU
  pair        xDct32FwdCtuFromTilesDev + xDct32InvCtuToTilesDev: the cheapest an unfused loop could be without a quantiser   48 KiB per CTU

each next to this box's copy stream (xHipMemCeilingDev X266_MEM_COPY) of its own bytes; a copy of B bytes moves 2 B, so the
stream copies half of them.  "of copy" = copy time / call time.  The fused call's outputs are compared with the chain's first.
Usage: gpu_quant.py [W H [QP]]   (default 3840 2176 27)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import x266_amd  # noqa: E402

ROUNDS, REPS = 20, 100
ROUNDING = 171


def trimmed_mean(v, frac=0.10):
    v = sorted(v)
    k = int(len(v) * frac)
    v = v[k:len(v) - k] if len(v) > 2 * k else v
    return sum(v) / len(v)


def main(argv):
    w, h = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (3840, 2176)
    qp = int(argv[2]) if len(argv) >= 3 else 27
    assert w % 64 == 0 and h % 64 == 0
    codec = x266_amd.Codec(0)
    ev = [codec.event_create() for _ in range(2)]
    print("device: %s" % (codec.device_info(),))
    n = codec.ctu_count(w, h)
    tile_bytes, level_bytes = w * h * 2, n * 12288
    # cur: random pixels; pred: cur plus a small difference, so that the residual looks like one (a few levels survive qp 27)
    rs = np.random.RandomState(0x266)
    cur_h = rs.randint(0, 256, tile_bytes).astype(np.uint8)
    pred_h = np.clip(cur_h.astype(np.int16) + rs.randint(-12, 13, tile_bytes), 0, 255).astype(np.uint8)
    cur, pred, pred_chain, recon = (codec.alloc(tile_bytes) for _ in range(4))
    cur.upload(cur_h)
    level, coef, lev2 = codec.alloc(level_bytes), codec.alloc(level_bytes), codec.alloc(level_bytes)
    nnz, nnz2 = codec.alloc(n * 24), codec.alloc(n * 24)
    copy_bytes = {"regions": n * 6 * 4096, "fused": n * 30720, "chain": n * 98304, "pair": n * 49152}
    half = max(copy_bytes.values()) // 2
    src, dst = codec.alloc(half), codec.alloc(half)
    codec.fill_residual_dev(src.ptr, half // 2, 0x71)

    def chain():
        codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred_chain.ptr, w, h, coef.ptr)
        codec.quant_regions_dev(0, coef.ptr, coef.ptr, 6 * n, 0, 0, qp, ROUNDING, nnz2.ptr)
        codec.quant_regions_dev(1, coef.ptr, coef.ptr, 6 * n, 0, 0, qp, ROUNDING)
        codec.dct32_inv_ctu_to_tiles_dev(coef.ptr, pred_chain.ptr, w, h, recon.ptr)

    # the fused call writes what the chain writes
    pred.upload(pred_h)
    pred_chain.upload(pred_h)
    codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred_chain.ptr, w, h, coef.ptr)
    codec.quant_regions_dev(0, coef.ptr, lev2.ptr, 6 * n, 0, 0, qp, ROUNDING, nnz2.ptr)
    chain()
    codec.dct32_code_ctu_tiles_dev(cur.ptr, pred.ptr, w, h, 0, qp, ROUNDING, level.ptr, nnz.ptr, pred.ptr)
    codec.stream_sync()
    lv = level.download(np.int16, n * 6144)
    assert np.array_equal(lv, lev2.download(np.int16, n * 6144)), "fused levels differ from the chain's"
    assert np.array_equal(nnz.download(np.uint32, n * 6), nnz2.download(np.uint32, n * 6)), "fused non-zero counts differ from the chain's"
    assert np.array_equal(pred.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384], recon.download(np.uint8, tile_bytes).reshape(-1, 512)[:, :384]), \
        "fused reconstruction differs from the chain's"
    print("fused == chain (levels, counts, m_Y / m_C); %.1f %% of the levels are non-zero at qp %d" % (100.0 * np.count_nonzero(lv) / lv.size, qp))
    pred.upload(pred_h)

    calls = {
        "regions": lambda: codec.quant_regions_dev(0, lev2.ptr, coef.ptr, 6 * n, 0, 0, qp, ROUNDING, nnz2.ptr),
        "fused": lambda: codec.dct32_code_ctu_tiles_dev(cur.ptr, pred.ptr, w, h, 0, qp, ROUNDING, level.ptr, nnz.ptr, recon.ptr),
        "chain": chain,
        "pair": lambda: (codec.dct32_fwd_ctu_from_tiles_dev(cur.ptr, pred_chain.ptr, w, h, coef.ptr),
                         codec.dct32_inv_ctu_to_tiles_dev(coef.ptr, pred_chain.ptr, w, h, recon.ptr)),
    }
    for k, nbytes in copy_bytes.items():
        calls["copy of the %s bytes" % k] = lambda nbytes=nbytes: codec.mem_ceiling_dev(0, src.ptr, dst.ptr, (nbytes // 2) & ~15)

    def timed(fn):
        codec.event_record(ev[0])
        for _ in range(REPS):
            fn()
        codec.event_record(ev[1])
        codec.stream_sync()
        return codec.event_elapsed_ms(ev[0], ev[1]) / REPS

    for fn in calls.values():                                           # warm-up: code objects, clocks
        for _ in range(3):
            fn()
    codec.stream_sync()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    t = {k: trimmed_mean(v) for k, v in ms.items()}
    print("\n%d x %d (%d CTUs, %d regions), qp %d, rounding %d: 10 %% trimmed mean of %d rounds x %d calls, all legs alternating"
          % (w, h, n, 6 * n, qp, ROUNDING, ROUNDS, REPS))
    print("%-28s %9s %9s %9s %10s %9s" % ("leg", "us", "min us", "max us", "TB/s", "of copy"))
    for k in calls:
        base = k[len("copy of the "):-len(" bytes")] if k.startswith("copy of") else k
        of = "" if k.startswith("copy of") else "%9.3f" % (t["copy of the %s bytes" % k] / t[k])
        print("%-28s %9.2f %9.2f %9.2f %10.3f %9s" % (k, t[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, copy_bytes[base] / (t[k] * 1e-3) / 1e12, of))
    print("fused / chain %.3f, fused / pair %.3f, fused / copy of its 30 KiB per CTU %.3f, chain / pair %.3f"
          % (t["fused"] / t["chain"], t["fused"] / t["pair"], t["fused"] / t["copy of the fused bytes"], t["chain"] / t["pair"]))
    print("the fused call %s than the four-call chain" % ("is faster" if t["fused"] < t["chain"] else "IS NOT FASTER"))
    for e in ev:
        codec.event_destroy(e)


if __name__ == "__main__":
    main(sys.argv[1:])
