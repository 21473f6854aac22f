"""The lookahead of include/x266hip.h (xLaDownscaleGpu, xLaIntraCostsGpu, xLaFrameCostGpu, xSceneCutFromTotals, xLaPropagateGpu,
xLaTreeQpGpu) restated from the header's text: the box filter and the intra costs in numpy, the per-block decisions, the propagation
and the qp map in plain loops over Python integers.  Also the frames the CPU and the GPU tests share.  tests/test_la_ref.py holds it
against the values the header states.  The qp bytes go through tests/_aq_ref.py's delta: that rule is stated once in the header."""
import numpy as np

import _aq_ref as A

BLOCK_DTYPE = np.dtype([("cost", "<u4"), ("intra", "<u4"), ("mvx", "<i2"), ("mvy", "<i2"), ("kind", "u1"), ("mode", "u1"), ("reserved", "<u2")])
ME_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("cost", "<u4")])
assert BLOCK_DTYPE.itemsize == 16 and ME_DTYPE.itemsize == 8
MODES = (0, 1, 10, 26)                                                      # planar, DC, horizontal, vertical: the order they are tried in
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
OFFSET_MAX = 3072


# ---- tiles <-> planes -----------------------------------------------------------------------------------------------------------------------
def planes_from_tiles(tiles, w, h):
    """(y [h, w], u, v [h / 2, w / 2]) of a tile array"""
    t = np.ascontiguousarray(tiles, np.uint8).reshape(h // 16, w // 16, 512)
    y = t[:, :, :256].reshape(h // 16, w // 16, 16, 16).transpose(0, 2, 1, 3).reshape(h, w)
    c = t[:, :, 256:384].reshape(h // 16, w // 16, 8, 8, 2).transpose(0, 2, 1, 3, 4).reshape(h // 2, w // 2, 2)
    return y, c[:, :, 0], c[:, :, 1]


def box(p):
    """the 2x2 box of a plane: (a + b + c + d + 2) >> 2"""
    p = np.asarray(p, np.int64)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def downscale(tiles, w, h, base=None):
    """the lowres tile array [n / 4, 512] of a full-resolution one; m_I is `base`'s (never written)"""
    y, u, v = planes_from_tiles(tiles, w, h)
    low = A.tiles_from_planes(box(y), box(u), box(v))
    if base is not None:
        low[:, 384:] = np.asarray(base, np.uint8).reshape(-1, 512)[:, 384:]
    return low


# ---- intra costs ----------------------------------------------------------------------------------------------------------------------------
def _h8():
    i = np.arange(8)
    return np.array([[(-1) ** bin(a & b).count("1") for b in i] for a in i], np.int64)


H8 = _h8()


def satd8x8(d):
    """(sum |H d H^T| + 2) >> 2 of one 8x8 difference"""
    return (int(np.abs(H8 @ np.asarray(d, np.int64) @ H8.T).sum()) + 2) >> 2


def neighbours(y, x0, y0):
    """(top[0..8], left[0..8]) of the 8x8 block at (x0, y0) of the lowres luma plane y"""
    hh, ww = y.shape
    if x0 == 0 and y0 == 0:
        return [128] * 9, [128] * 9
    top = [int(y[y0 - 1, min(x0 + i, ww - 1)]) for i in range(9)] if y0 else None
    left = [int(y[min(y0 + i, hh - 1), x0 - 1]) for i in range(9)] if x0 else None
    if top is None:
        top = [left[0]] * 9
    if left is None:
        left = [top[0]] * 9
    return top, left


def predictions(top, left):
    """the four candidates in the order they are tried"""
    tr, bl = top[8], left[8]
    x, yy = np.meshgrid(np.arange(8), np.arange(8))
    t, l = np.array(top[:8], np.int64), np.array(left[:8], np.int64)
    planar = ((7 - x) * l[yy] + (x + 1) * tr + (7 - yy) * t[x] + (yy + 1) * bl + 8) >> 4
    dc = np.full((8, 8), (int(t.sum()) + int(l.sum()) + 8) >> 4, np.int64)
    return [planar, dc, l[yy], t[x]]


def block_costs(y, x0, y0):
    """the four costs of one block, in candidate order"""
    cur = y[y0:y0 + 8, x0:x0 + 8].astype(np.int64)
    return [satd8x8(cur - p) for p in predictions(*neighbours(y, x0, y0))]


def intra_costs(low_tiles, w, h):
    """(d_intra uint32 [n], d_mode uint8 [n]) of the lowres frame of a w x h full-resolution frame"""
    y, _, _ = planes_from_tiles(low_tiles, w // 2, h // 2)
    bw, bh = w // 16, h // 16
    cost, mode = np.zeros(bw * bh, np.uint32), np.zeros(bw * bh, np.uint8)
    for by in range(bh):
        for bx in range(bw):
            c = block_costs(y, 8 * bx, 8 * by)
            k = c.index(min(c))                                             # the first of equal costs
            cost[by * bw + bx], mode[by * bw + bx] = c[k], MODES[k]
    return cost, mode


# ---- frame cost -----------------------------------------------------------------------------------------------------------------------------
def frame_cost(intra, mode, inter0, inter1, intra_penalty):
    """(records [n] of BLOCK_DTYPE, totals int64 [8]); mode, inter0, inter1 may be None"""
    n = len(intra)
    rec, tot = np.zeros(n, BLOCK_DTYPE), np.zeros(8, np.int64)
    for b in range(n):
        ci = (int(intra[b]) + intra_penalty) & M32
        best = None
        if inter0 is not None:
            best = (int(inter0["cost"][b]), 1, inter0[b])
        if inter1 is not None and (best is None or int(inter1["cost"][b]) < best[0]):
            best = (int(inter1["cost"][b]), 2, inter1[b])
        if best is None or ci < best[0]:
            best = (ci, 0, None)
        rec[b] = (best[0], intra[b], best[2]["mvx"] if best[1] else 0, best[2]["mvy"] if best[1] else 0, best[1], 0 if mode is None else mode[b], 0)
        tot[0] += best[0]
        tot[1] += int(intra[b])
        tot[2 + best[1]] += 1
        tot[5] += 0 if inter0 is None else int(inter0["cost"][b])
        tot[6] += 0 if inter1 is None else int(inter1["cost"][b])
    tot[7] = n
    return rec, tot


def scene_cut_bias(threshold_q8, g, min_keyint, max_keyint):
    tmax = threshold_q8 << 8
    tmin = tmax >> 2
    if 4 * g <= min_keyint:
        return tmin >> 2
    if g <= min_keyint:
        return tmin * g // min_keyint
    if max_keyint == min_keyint:
        return tmax
    return tmin + (tmax - tmin) * (g - min_keyint) // (max_keyint - min_keyint)


def scene_cut(total, threshold_q8, g, min_keyint, max_keyint):
    if total is None or not 0 <= threshold_q8 <= 256 or g < 0 or min_keyint < 1 or max_keyint < min_keyint:
        return -1
    if any(int(t) < 0 for t in total) or not 1 <= int(total[7]) <= 1 << 24 or int(total[0]) > 1 << 40 or int(total[1]) > 1 << 40:
        return -1
    return 1 if int(total[0]) * 65536 >= (65536 - scene_cut_bias(threshold_q8, g, min_keyint, max_keyint)) * int(total[1]) else 0


# ---- the propagation tree -------------------------------------------------------------------------------------------------------------------
def amount(cost, intra, prop):
    q = min(int(prop), M32)
    inter = min(int(cost), int(intra))
    return (((int(intra) + q) * (int(intra) - inter)) & M64) // int(intra)


def targets(bx, by, mvx, mvy):
    """[(X, Y, weight)] of the four targets, the grid not yet looked at"""
    px, py = 8 * bx + int(mvx), 8 * by + int(mvy)
    X, Y = px // 8, py // 8                                                  # Python's // is floor division
    dx, dy = px - 8 * X, py - 8 * Y
    return [(X, Y, (8 - dx) * (8 - dy)), (X + 1, Y, dx * (8 - dy)), (X, Y + 1, (8 - dx) * dy), (X + 1, Y + 1, dx * dy)]


def propagate(rec, prop, ref0, ref1, w, h):
    """one step: adds into the Python-integer lists ref0 and ref1 (either may be None) and returns them as uint64 arrays"""
    bw, bh = w // 16, h // 16
    acc = [None if r is None else [int(v) for v in r] for r in (ref0, ref1)]
    for b in range(bw * bh):
        kind, intra = int(rec["kind"][b]), int(rec["intra"][b])
        if kind == 0 or intra == 0 or acc[kind - 1] is None:
            continue
        a = amount(rec["cost"][b], intra, 0 if prop is None else prop[b])
        for X, Y, wgt in targets(b % bw, b // bw, rec["mvx"][b], rec["mvy"][b]):
            if wgt > 0 and 0 <= X < bw and 0 <= Y < bh:
                acc[kind - 1][Y * bw + X] = (acc[kind - 1][Y * bw + X] + ((a * wgt + 32) >> 6)) & M64
    return [None if a is None else np.array(a, np.uint64) for a in acc]


def gain(intra, prop, strength_q8):
    intra = int(intra)
    if intra == 0:
        return 0
    p = min(int(prop), M32 - intra)
    return (strength_q8 * (int(A.log2_q8(intra + p)) - int(A.log2_q8(intra)))) >> 8


def tree_offsets(rec, prop, aq_offset, strength_q8):
    n = rec.size
    off = np.zeros(n, np.int64)
    for t in range(n):
        aq = 0 if aq_offset is None else int(aq_offset[t])
        off[t] = min(max(aq - gain(rec["intra"][t], 0 if prop is None else prop[t], strength_q8), -OFFSET_MAX), OFFSET_MAX)
    return off


def region_qp(off, w, h, qp, chroma_qp_offset):
    """the qp bytes of tile offsets, by the rule of the source analysis"""
    tw, th = w // 16, h // 16
    cw, ch = (w + 63) // 64, (h + 63) // 64
    out = np.zeros(6 * cw * ch, np.uint8)
    for cy in range(ch):
        for cx in range(cw):
            s, n = [0] * 4, [0] * 4
            for ty in range(4 * cy, min(4 * cy + 4, th)):
                for tx in range(4 * cx, min(4 * cx + 4, tw)):
                    q = ((ty >> 1) & 1) * 2 + ((tx >> 1) & 1)
                    s[q] += int(off[ty * tw + tx])
                    n[q] += 1
            for q in range(6):
                d = A.delta(s[q], n[q]) if q < 4 else A.delta(sum(s), sum(n))
                out[6 * (cy * cw + cx) + q] = min(max(qp + d + (chroma_qp_offset if q >= 4 else 0), 0), 51)
    return out


def tree_qp(rec, prop, aq_offset, w, h, strength_q8, qp, chroma_qp_offset):
    """(Q8 offsets int16 [n], qp bytes uint8 [6 n_ctu])"""
    off = tree_offsets(rec, prop, aq_offset, strength_q8)
    return off.astype(np.int16), region_qp(off, w, h, qp, chroma_qp_offset)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def frame(kind, w, h, seed=0):
    """a tile array [n, 512] of a w x h frame; m_I is seeded garbage"""
    r = np.random.RandomState(0x1A00 + seed + w + 7 * h)
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    if kind == "zeros":
        y = np.zeros((h, w))
    elif kind == "ones":
        y = np.full((h, w), 255)
    elif kind == "random":
        y = r.randint(0, 256, (h, w))
    elif kind == "hramp":
        y = (xx * 5) % 256
    elif kind == "vramp":
        y = (yy * 3) % 256
    elif kind == "checker":                                                 # 0 / 255 per lowres sample: it survives the box filter
        y = 255 * (((xx >> 1) + (yy >> 1)) & 1)
    else:                                                                   # "smooth": something a search can follow
        y = 128 + 60 * np.sin(xx / 9.0) + 50 * np.cos(yy / 7.0) + r.randint(-4, 5, (h, w))
    y = np.clip(y, 0, 255).astype(np.uint8)
    c = r.randint(0, 256, (2, h // 2, w // 2)) if kind == "random" else np.stack([y[::2, ::2] // 2 + 30, 255 - y[1::2, 1::2]])
    if kind in ("zeros", "ones"):
        c = np.stack([y[::2, ::2], y[::2, ::2]])
    return A.tiles_from_planes(y, c[0], c[1], seed + 3)


def shifted(tiles, w, h, dx, dy):
    """the frame moved by (dx, dy) full-resolution samples, edges replicated"""
    y, u, v = planes_from_tiles(tiles, w, h)
    mv = lambda p, sx, sy: np.pad(p, ((abs(sy), abs(sy)), (abs(sx), abs(sx))), mode="edge")[abs(sy) - sy:abs(sy) - sy + p.shape[0], abs(sx) - sx:abs(sx) - sx + p.shape[1]]
    return A.tiles_from_planes(mv(y, dx, dy), mv(u, dx // 2, dy // 2), mv(v, dx // 2, dy // 2), 5)


def search(cur_low, ref_low, w, h, rng):
    """the full SATD search of two lowres frames (of a w x h full-resolution pair): records [n] of ME_DTYPE; first in raster order wins"""
    cy, _, _ = planes_from_tiles(cur_low, w // 2, h // 2)
    ry, _, _ = planes_from_tiles(ref_low, w // 2, h // 2)
    pad = np.pad(ry, rng, mode="edge").astype(np.int64)
    bw, bh = w // 16, h // 16
    out = np.zeros(bw * bh, ME_DTYPE)
    for by in range(bh):
        for bx in range(bw):
            cur = cy[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.int64)
            best = None
            for dy in range(-rng, rng + 1):
                for dx in range(-rng, rng + 1):
                    c = satd8x8(cur - pad[8 * by + dy + rng:8 * by + dy + rng + 8, 8 * bx + dx + rng:8 * bx + dx + rng + 8])
                    if best is None or c < best[2]:
                        best = (dx, dy, c)
            out[by * bw + bx] = best
    return out


def lists(intra, seed):
    """two lists' records built around the intra costs so that every branch of the decision occurs, ties included"""
    n, r = intra.size, np.random.RandomState(seed)
    l0, l1 = np.zeros(n, ME_DTYPE), np.zeros(n, ME_DTYPE)
    for a in (l0, l1):
        a["mvx"], a["mvy"] = r.randint(-64, 65, n), r.randint(-64, 65, n)
        a["cost"] = np.maximum(intra.astype(np.int64) + r.randint(-300, 901, n), 0)   # around intra + the penalty of 300
    k = np.arange(n) % 8
    l1["cost"][k == 1] = l0["cost"][k == 1]                                  # list 1 ties with list 0
    l0["cost"][k == 2] = intra[k == 2] + 300                                # intra (penalty 300) ties with list 0 ...
    l1["cost"][k == 3] = intra[k == 3] + 300                                # ... and with list 1
    l0["cost"][k == 4] = l1["cost"][k == 4] = intra[k == 4] + 300          # all three tie
    return l0, l1
