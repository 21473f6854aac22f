"""The statement of xTransformDecideCtuTilesGpu (include/x266hip.h), by composition of the committed references: the CTU-ordered
residual of two tiled frames (the statement of xTransformCtuFromTilesDev in test_gpu_transform_ctu_tiles.py), the oracle's forward
transforms per class (transform_fwd / dct32_fwd, or the installed matrices) and _rdoq_ref.rdo_quant.  Nothing here restates a
transform, a rate table or a scan.  Also the synthetic content the CPU and the GPU tests share."""
import numpy as np

import _rdoq_ref as rref
from _quant_ref import region_qp
from test_gpu_transform_ctu_tiles import _class_transform, _planes, _regions_of_planes, _to_blocks

CLASSES = 0x777F                                                         # X266_TDECIDE_CLASSES
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
CLASS_LIST = [k for k in range(16) if (CLASSES >> k) & 1]


def n_regions(w, h):
    return 6 * ((w + 63) // 64) * ((h + 63) // 64)


def effective_masks(n, cand_luma=CLASSES, cand_chroma=CLASSES, cand=None):
    """[n] the mask each region decides over: d_cand[r] & 0x777F when that is non-zero, else cand_luma (q < 4) / cand_chroma"""
    base = np.where(np.arange(n) % 6 < 4, cand_luma, cand_chroma).astype(np.int64)
    if cand is None:
        return base
    own = np.asarray(cand, np.uint16).ravel().astype(np.int64) & CLASSES
    assert own.size == n
    return np.where(own != 0, own, base)


def residual_regions(cur, pred, w, h):
    """[n, 32, 32] int16: cur - pred per region (6 ctu + q), zero outside the frame"""
    cy, cu, cv = _planes(cur, w, h)
    py, pu, pv = _planes(pred, w, h)
    d = lambda a, b: a.astype(np.int16) - b.astype(np.int16)
    return _regions_of_planes(d(cy, py), d(cu, pu), d(cv, pv), w, h).reshape(-1, 32, 32)


def decide_regions(oracle, res, masks, qp_of, lam, class_bits=None, mats=None):
    """res [m, 32, 32] int16 residual regions, their masks and qps -> (class bytes uint8 [m], levels int16 [m, 1024], records
    STAT_DTYPE [m], costs uint64 [m, 16]); python integers hold every J"""
    res = np.asarray(res, np.int16).reshape(-1, 32, 32)
    m = res.shape[0]
    masks = np.asarray(masks).ravel().astype(np.int64)
    qp_of = np.asarray(qp_of).ravel().astype(np.int64)
    bits = [0] * 16 if class_bits is None else [int(b) for b in class_bits] + [0] * (16 - len(class_bits))
    assert masks.size == m and qp_of.size == m and np.all(masks & ~CLASSES == 0) and np.all(masks != 0)
    cls = np.zeros(m, np.uint8)
    levels = np.zeros((m, 1024), np.int16)
    stat = np.zeros(m, rref.STAT_DTYPE)
    cost = np.full((m, 16), ALL_ONES, np.uint64)
    best = [None] * m
    for k in CLASS_LIST:                                                 # ascending: "<" keeps the smallest class byte on a tie
        sel = np.flatnonzero((masks >> k) & 1)
        if sel.size == 0:
            continue
        c_k = _class_transform(oracle, k, _to_blocks(res[sel], 4 << (k & 3)), False, mats)
        l_k, s_k, _ = rref.rdo_quant(c_k, classes=np.full(sel.size, k, np.uint8), qps=qp_of[sel].astype(np.uint8), lam=lam)
        for i, r in enumerate(sel):
            j = int(s_k["dist"][i]) + lam * (int(s_k["bits"][i]) + bits[k])
            assert j < (1 << 64) - 1
            cost[r, k] = np.uint64(j)
            if best[r] is None or j < best[r]:
                best[r], cls[r], levels[r], stat[r] = j, k, l_k[i], s_k[i]
    return cls, levels, stat, cost


def decide(oracle, cur, pred, w, h, qps=None, qp=0, lam=368, cand_luma=CLASSES, cand_chroma=CLASSES, cand=None, class_bits=None, mats=None,
           regions=None):
    """the call on a frame; `regions`: the region indices to decide (None: all of them) -> the outputs for those regions, in that order"""
    n = n_regions(w, h)
    sel = np.arange(n) if regions is None else np.asarray(regions, np.int64)
    res = residual_regions(cur, pred, w, h)[sel]
    return decide_regions(oracle, res, effective_masks(n, cand_luma, cand_chroma, cand)[sel], region_qp(qps, qp, n)[sel], lam, class_bits, mats)


# ---- the content the CPU and the GPU tests share -----------------------------------------------------------------------------------------
KINDS = ("sinusoid", "edge", "ramp8", "noise6", "spot")


def content(kind, seed=7):
    """one 32x32 int16 residual of the named kind, every value within -255..255"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:32, 0:32]
    if kind == "sinusoid":
        return np.rint(60.0 * np.cos(np.pi * (x + 0.5) / 32.0) * np.cos(np.pi * (y + 0.5) / 64.0)).astype(np.int16)
    if kind == "edge":
        return np.where(x < 13, 50, -40).astype(np.int16)
    if kind == "ramp8":
        return (((x + y) % 8) * 10 - 35).astype(np.int16)
    if kind == "noise6":
        return rng.randint(-6, 7, (32, 32)).astype(np.int16)
    if kind == "spot":
        r = rng.randint(-1, 2, (32, 32)).astype(np.int16)
        r[8:12, 20:24] = np.where(rng.randint(0, 2, (4, 4)) == 1, 60, -60)
        return r
    raise ValueError(kind)


def tiles_of_planes(oracle, y, u, v):
    return oracle.conv_input_fmt(np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(u, np.uint8), np.ascontiguousarray(v, np.uint8)).ravel()


def content_frames(oracle, w, h, seed=3):
    """(cur, pred) tile arrays of a w x h frame whose residual is the five kinds tiled over 32x32 cells of luma and chroma, the kind
    of a cell chosen by (cell row + cell column + seed) % 5; pred is flat 128"""
    def plane(ph, pw, shift):
        out = np.zeros((ph, pw), np.int16)
        for cy in range(0, ph, 32):
            for cx in range(0, pw, 32):
                cell = content(KINDS[(cy // 32 + cx // 32 + seed + shift) % 5], seed + cy + cx)
                out[cy:cy + 32, cx:cx + 32] = cell[:min(32, ph - cy), :min(32, pw - cx)]
        return out
    res = plane(h, w, 0), plane(h // 2, w // 2, 1), plane(h // 2, w // 2, 2)
    pred = [np.full(r.shape, 128, np.uint8) for r in res]
    cur = [np.clip(r + 128, 0, 255).astype(np.uint8) for r in res]
    return tiles_of_planes(oracle, *cur), tiles_of_planes(oracle, *pred)


def encoder_masks(w, h, luma=CLASSES, chroma=CLASSES):
    """uint16 [n]: per-region masks that keep N from straddling the frame edge: N <= 16 where a region's in-frame extent is 16 in
    either direction, N <= 8 where it is 8 or 24 (chroma of frames that are an odd multiple of 16); 0 (fall back to the scalar masks)
    for whole regions and for regions wholly outside the frame"""
    nx, ny = (w + 63) // 64, (h + 63) // 64
    size_mask = {32: CLASSES, 16: 0x7777, 8: 0x3333}
    out = np.zeros((ny, nx, 6), np.uint16)
    for cy in range(ny):
        for cx in range(nx):
            for q in range(6):
                if q < 4:
                    ex, ey = np.clip(w - (cx * 64 + (q & 1) * 32), 0, 32), np.clip(h - (cy * 64 + (q >> 1) * 32), 0, 32)
                else:
                    ex, ey = np.clip(w // 2 - cx * 32, 0, 32), np.clip(h // 2 - cy * 32, 0, 32)
                if ex == 0 or ey == 0 or (ex == 32 and ey == 32):
                    continue
                lim = 32
                for e in (ex, ey):
                    lim = min(lim, 32 if e == 32 else 16 if e == 16 else 8)
                out[cy, cx, q] = (luma if q < 4 else chroma) & size_mask[lim]
    return out.ravel()
