"""Frame quality of include/x266hip.h (xQualityStatsGpu, xQualityFromTotals) restated from the header's text: squared errors and 4x4
block sums in numpy int64, every window in Python integers, PSNR and SSIM in numpy float64.  Also the frame pairs the CPU and the GPU
tests share.  tests/test_quality_ref.py holds it against the values the header states and against the same formula in float64."""
import numpy as np

from _aq_ref import tiles_from_planes

SSE, SSIM = 1, 2
C1, C2 = 416, 235963
ONE = 1 << 30
CTU_DTYPE = np.dtype([("ssim", "<i8", (3,)), ("sse", "<u4", (3,)), ("win_y", "<u4"), ("win_c", "<u4"), ("reserved", "<u4")])
assert CTU_DTYPE.itemsize == 48


def window(s1, s2, ss, s12):
    """(q, cn, exact) of a window from its four sums, in Python integers; exact: cn's quotient is an integer (truncation = floor)"""
    s1, s2, ss, s12 = int(s1), int(s2), int(ss), int(s12)
    var, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    ln, ld = 2 * s1 * s2 + C1, s1 * s1 + s2 * s2 + C1
    cn, cd = 2 * covar + C2, var + C2
    assert 0 < ln <= ld and abs(cn) <= cd and (max(ln, abs(cn)) << 30) < (1 << 61)
    lq = (ln << 30) // ld
    cm = (abs(cn) << 30) // cd                                              # toward zero
    cq = -cm if cn < 0 else cm
    return (lq * cq) >> 30, cn, (abs(cn) << 30) % cd == 0                   # Python's >> floors


def window_float(s1, s2, ss, s12):
    """the same formula in float64: the SSIM of the window"""
    s1, s2, ss, s12 = float(s1), float(s2), float(ss), float(s12)
    var, covar = 64.0 * ss - s1 * s1 - s2 * s2, 64.0 * s12 - s1 * s2
    return (2.0 * s1 * s2 + C1) * (2.0 * covar + C2) / ((s1 * s1 + s2 * s2 + C1) * (var + C2))


def sums_of(a, b):
    """(S1, S2, SS, S12) of two sample arrays of any one shape"""
    a, b = np.asarray(a, np.int64).ravel(), np.asarray(b, np.int64).ravel()
    return int(a.sum()), int(b.sum()), int((a * a + b * b).sum()), int((a * b).sum())


def planes_from_tiles(tiles, w, h):
    """(y [h, w], u, v [h / 2, w / 2]) of a tile array; m_I is not looked at"""
    th, tw = h // 16, w // 16
    t = np.ascontiguousarray(tiles, np.uint8).reshape(th, tw, 512)
    y = t[:, :, :256].reshape(th, tw, 16, 16).transpose(0, 2, 1, 3).reshape(h, w)
    c = t[:, :, 256:384].reshape(th, tw, 8, 8, 2).transpose(0, 2, 1, 3, 4).reshape(h // 2, w // 2, 2)
    return y, c[:, :, 0], c[:, :, 1]


def window_sums(a, b):
    """the four sums of every window of a plane pair, int64 [H4 - 1, W4 - 1] each: 4x4 block sums, then 2x2 blocks"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    h4, w4 = a.shape[0] // 4, a.shape[1] // 4
    blocks = lambda x: x.reshape(h4, 4, w4, 4).sum((1, 3))
    out = []
    for x in (a, b, a * a + b * b, a * b):
        s = blocks(x)
        out.append(s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:])
    return out


def border_kind(bx, by, plane):
    """(x, y) with 0: the window lies inside one tile on that axis, 1: it crosses a tile border, 2: a CTU border"""
    per_tile, per_ctu = (4, 16) if plane == 0 else (2, 8)
    kind = lambda b: 2 if b % per_ctu == per_ctu - 1 else 1 if b % per_tile == per_tile - 1 else 0
    return kind(bx), kind(by)


def stats(src_tiles, dec_tiles, w, h, flags=SSE | SSIM, counters=None):
    """the records [n_ctu] of CTU_DTYPE.  counters: a dict that receives "inexact_negative" (windows with cn < 0 whose quotient is
    not an integer), "kinds" ({plane: set of border_kind}) and "q" ({plane: int64 [H4 - 1, W4 - 1]})"""
    assert w > 0 and h > 0 and w % 16 == 0 and h % 16 == 0 and flags in (1, 2, 3)
    cw, ch = (w + 63) // 64, (h + 63) // 64
    rec = np.zeros(cw * ch, CTU_DTYPE)
    pa, pb = planes_from_tiles(src_tiles, w, h), planes_from_tiles(dec_tiles, w, h)
    inexact, kinds, qs = 0, {}, {}
    for p in range(3):
        a, b = pa[p].astype(np.int64), pb[p].astype(np.int64)
        edge = 64 if p == 0 else 32                                           # a CTU's side in this plane's samples
        if flags & SSE:
            d = np.zeros((ch * edge, cw * edge), np.int64)
            d[:a.shape[0], :a.shape[1]] = (a - b) ** 2
            rec["sse"][:, p] = d.reshape(ch, edge, cw, edge).sum((1, 3)).ravel()
        if flags & SSIM:
            s1, s2, ss, s12 = window_sums(a, b)
            shift = 4 if p == 0 else 3
            q_all = np.zeros(s1.shape, np.int64)
            kinds[p] = set()
            for by in range(s1.shape[0]):
                for bx in range(s1.shape[1]):
                    q, cn, exact = window(s1[by, bx], s2[by, bx], ss[by, bx], s12[by, bx])
                    inexact += cn < 0 and not exact
                    kinds[p].add(border_kind(bx, by, p))
                    q_all[by, bx] = q
                    rec["ssim"][(by >> shift) * cw + (bx >> shift), p] += q
                    if p < 2:
                        rec["win_y" if p == 0 else "win_c"][(by >> shift) * cw + (bx >> shift)] += 1
            qs[p] = q_all
    if counters is not None:
        counters.update(inexact_negative=inexact, kinds=kinds, q=qs)
    return rec


def totals(rec):
    """d_total[8]: sse Y, U, V, ssim Y, U, V, win_y, win_c over all records"""
    out = np.zeros(8, np.int64)
    out[0:3] = rec["sse"].astype(np.int64).sum(0)
    out[3:6] = rec["ssim"].sum(0)
    out[6], out[7] = int(rec["win_y"].astype(np.int64).sum()), int(rec["win_c"].astype(np.int64).sum())
    return out


def window_counts(w, h):
    """(win_y, win_c) of a w x h frame"""
    return (w // 4 - 1) * (h // 4 - 1), (w // 8 - 1) * (h // 8 - 1)


def from_totals(total, w, h):
    """(psnr [4], ssim [3]) in numpy float64"""
    t = np.asarray(total, np.int64)
    n = np.array([w * h, w * h / 4, w * h / 4], np.float64)
    sse = t[:3].astype(np.float64)
    one = lambda e, m: np.float64(100.0) if e == 0 else np.float64(10.0) * np.log10(np.float64(65025.0) * m / e)
    psnr = np.array([one(sse[p], n[p]) for p in range(3)] + [one(sse[0] + sse[1] + sse[2], n[0] + n[1] + n[2])], np.float64)
    win = np.array([t[6], t[7], t[7]], np.float64)
    ssim = np.array([1.0 if win[p] == 0 else np.float64(t[3 + p]) / (win[p] * np.float64(ONE)) for p in range(3)], np.float64)
    return psnr, ssim


# ---- frame pairs ----------------------------------------------------------------------------------------------------------------------------
def _planes(w, h, seed):
    r = np.random.RandomState(seed)
    return [r.randint(0, 256, (h, w)), r.randint(0, 256, (h // 2, w // 2)), r.randint(0, 256, (h // 2, w // 2))]


def _ramp(w, h, seed):
    """a smooth ramp plus a little noise: what a coded frame looks like to the structure term"""
    r = np.random.RandomState(seed)
    out = []
    for hh, ww, k in ((h, w, 1), (h // 2, w // 2, 2), (h // 2, w // 2, 3)):
        base = 40 * k + (np.arange(hh)[:, None] * 3 + np.arange(ww)[None, :] * 2) // (2 * k)
        out.append(np.clip(base % 224 + r.randint(-4, 5, (hh, ww)), 0, 255))
    return out


def pair(kind, w, h, seed=0):
    """(src tiles, dec tiles) [n_tiles, 512] uint8; the two frames' m_I bytes are different garbage"""
    if kind == "same":
        a = b = _planes(w, h, seed)
    elif kind == "extremes":
        a = [np.zeros((h, w)), np.zeros((h // 2, w // 2)), np.zeros((h // 2, w // 2))]
        b = [x + 255 for x in a]
    elif kind == "noise":
        a, b = _planes(w, h, seed), _planes(w, h, seed + 1000)
    elif kind == "inverse":
        a = _planes(w, h, seed)
        b = [255 - x for x in a]
    elif kind == "distorted":
        a = _ramp(w, h, seed)
        r = np.random.RandomState(seed + 7)
        b = [np.clip(x + r.randint(-3, 4, x.shape), 0, 255) for x in a]
    else:
        raise ValueError(kind)
    return tiles_from_planes(*a, seed=seed + 1), tiles_from_planes(*b, seed=seed + 2)
