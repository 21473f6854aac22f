#!/usr/bin/env python3
"""Developer probe: same-box A/B of the from-tiles calls -- xSatd8x8FromTilesDev, xDct32FwdFromTilesDev, xDct32FwdChromaFromTilesDev,
xDct32FwdCtuFromTilesDev -- between tools/_ab/libx266hip_ref.so (tools/ab_build.sh <git-ref>) and the working tree's library."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p; SZ = ctypes.c_size_t
def load(path):
    L = ctypes.CDLL(path); ctx = P()
    assert L.xHipCodecInit(ctypes.byref(ctx), 0) == 0
    L.xHipMalloc.argtypes = [P, ctypes.POINTER(P), SZ]
    L.xFillResidualDev.argtypes = [P, P, SZ, ctypes.c_uint64, ctypes.c_uint64, P]
    L.xHipStreamSync.argtypes = [P, P]
    L.xHipEventCreate.argtypes = [P, ctypes.POINTER(P)]
    L.xHipEventRecord.argtypes = [P, P, P]
    L.xHipEventElapsedMs.argtypes = [P, P, P, ctypes.POINTER(ctypes.c_double)]
    L.xSatd8x8FromTilesDev.argtypes = L.xDct32FwdFromTilesDev.argtypes = L.xDct32FwdCtuFromTilesDev.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, P, P]
    L.xDct32FwdChromaFromTilesDev.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, P, P, SZ, P]
    ev = [P() for _ in range(2)]
    for e in ev: assert L.xHipEventCreate(ctx, ctypes.byref(e)) == 0
    return L, ctx, ev
libs = [("ref", load(ROOT + "/tools/_ab/libx266hip_ref.so")), ("new", load(ROOT + "/x266_amd/libx266hip.so"))]
w = h = 32768
nt = (w // 16) * (h // 16)
L0, c0, _ = libs[0][1]
cur, pred, out = P(), P(), P()
for b, n in ((cur, nt * 512), (pred, nt * 512), (out, w * h // 64 * 4)): assert L0.xHipMalloc(c0, ctypes.byref(b), n) == 0
L0.xFillResidualDev(c0, cur, nt * 256, 1, 0, None); L0.xFillResidualDev(c0, pred, nt * 256, 2, 0, None); L0.xHipStreamSync(c0, None)
coef = P()
assert L0.xHipMalloc(c0, ctypes.byref(coef), w * h * 3) == 0                  # 12 KiB per CTU: luma, U, V coefficients
calls = [("satd8x8 from tiles", w * h // 64 * 132, lambda L, c: L.xSatd8x8FromTilesDev(c, cur, pred, w, h, out, None)),
         ("dct32 from tiles", w * h * 3, lambda L, c: L.xDct32FwdFromTilesDev(c, cur, pred, w, h, coef, None)),
         ("dct32 chroma from tiles", w * h * 2, lambda L, c: L.xDct32FwdChromaFromTilesDev(c, cur, pred, w, h, coef, P(coef.value + 2048), 2, None)),
         ("dct32 ctu from tiles", w * h * 5, lambda L, c: L.xDct32FwdCtuFromTilesDev(c, cur, pred, w, h, coef, None))]
def timed(L, ctx, ev, fn, reps=30):
    for _ in range(5): assert fn(L, ctx) == 0
    ms = ctypes.c_double()
    L.xHipEventRecord(ctx, ev[0], None)
    for _ in range(reps): fn(L, ctx)
    L.xHipEventRecord(ctx, ev[1], None); L.xHipStreamSync(ctx, None)
    L.xHipEventElapsedMs(ctx, ev[0], ev[1], ctypes.byref(ms)); return ms.value / reps
for tag, (L, c, ev) in libs: timed(L, c, ev, calls[0][2], 100)
for name, nbytes, fn in calls:
    best = {"ref": [], "new": []}
    for rnd in range(6):
        for tag, (L, c, ev) in libs: best[tag].append(timed(L, c, ev, fn))
    for tag in best: print("%-24s" % name, tag, "min %.4f mean %.4f ms" % (min(best[tag]), sum(best[tag]) / 6), "frac at mean %.3f" % (nbytes / (sum(best[tag]) / 6) / 8e9))
    print("%-24s new/ref time %.4f" % (name, min(best["new"]) / min(best["ref"])), flush=True)
