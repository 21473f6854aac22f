"""The reference statement of sample adaptive offset (include/x266hip.h: xSaoStatsGpu / DecideGpu / SearchGpu / ApplyGpu) in numpy int64
over the planes that oracle.conv_output_420 unpacks, and the data recipe of its test cases.  Nothing here is derived from the library
under test; tests/test_sao_ref.py holds it against a plain-loop evaluation of the header's text.

Categories: EO class k has the neighbours a, b = NEIGHBOURS[k] (dx, dy); one of them outside the plane: category 0; otherwise
sign(c - a) + sign(c - b) = -2, -1, 0, 1, 2 -> category 1, 2, 0, 3, 4.  Band = c >> 3.  Bins per CTU and component: 4 k + cat - 1, then
16 + band; (count, sum of org - dec).  Decision and apply: see the header."""
import collections

import numpy as np

from _util import splitmix64

NEIGHBOURS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))
CATEGORY_OF_SUM = np.array([1, 2, 0, 3, 4], np.int64)                     # index: sign sum + 2
BINS = 48
OFF, BO, EO = 0, 1, 2


def ctus(w, h):
    return (w + 63) // 64, (h + 63) // 64


# ---- categories -----------------------------------------------------------------------------------------------------------------------
def categories(plane):
    """[4, PH, PW]: the category of every sample for the four EO classes"""
    p = np.asarray(plane, np.int64)
    ph, pw = p.shape
    big = np.pad(p, 1)
    inside = np.pad(np.ones((ph, pw), bool), 1)
    out = np.zeros((4, ph, pw), np.int64)
    for k, (a, b) in enumerate(NEIGHBOURS):
        s = np.zeros((ph, pw), np.int64)
        ok = np.ones((ph, pw), bool)
        for dx, dy in (a, b):
            s += np.sign(p - big[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw])
            ok &= inside[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw]
        out[k] = np.where(ok, CATEGORY_OF_SUM[s + 2], 0)
    return out


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def stats_plane(org, dec, edge):
    """[ctus_y, ctus_x, 48, 2] int64 of one plane cut into edge x edge CTU components"""
    org, dec = np.asarray(org, np.int64), np.asarray(dec, np.int64)
    ph, pw = dec.shape
    cat, diff, band = categories(dec), org - dec, dec >> 3
    ny, nx = (ph + edge - 1) // edge, (pw + edge - 1) // edge
    out = np.zeros((ny, nx, BINS, 2), np.int64)
    for cy in range(ny):
        for cx in range(nx):
            win = (slice(cy * edge, (cy + 1) * edge), slice(cx * edge, (cx + 1) * edge))
            d = diff[win].ravel()
            for k in range(4):
                c = cat[k][win].ravel()
                for q in range(1, 5):
                    out[cy, cx, 4 * k + q - 1] = ((c == q).sum(), d[c == q].sum())
            b = band[win].ravel()
            out[cy, cx, 16:, 0] = np.bincount(b, minlength=32)
            out[cy, cx, 16:, 1] = np.bincount(b, weights=d, minlength=32).astype(np.int64)
    return out


def stats(org_planes, dec_planes):
    """(y, u, v) of org and dec -> d_stats as [n_ctu, 3, 48, 2] int64"""
    parts = [stats_plane(o, d, 64 if m == 0 else 32) for m, (o, d) in enumerate(zip(org_planes, dec_planes))]
    return np.stack([p.reshape(-1, BINS, 2) for p in parts], axis=1)


# ---- decision -------------------------------------------------------------------------------------------------------------------------
def rate(h, band):
    return np.minimum(np.abs(h) + 1, 7) + (band & (h != 0))


def offset_search(n, e, lo, hi, lam, band, info=None):
    """per bin (arrays of one shape): (offset, cost)"""
    n, e = np.asarray(n, np.int64), np.asarray(e, np.int64)
    h0 = np.where(n > 0, np.sign(e) * ((2 * np.abs(e) + n) // np.maximum(2 * n, 1)), 0)
    unclamped = h0
    h0 = np.clip(h0, lo, hi)
    cost = lambda h: 16 * (n * h * h - 2 * h * e) + lam * rate(h, band)
    best, best_cost = h0.copy(), cost(h0)
    for i in range(1, 8):
        h = h0 - np.sign(h0) * i
        c = cost(h)
        take = (i <= np.abs(h0)) & (c <= best_cost)
        best, best_cost = np.where(take, h, best), np.where(take, c, best_cost)
    if info is not None:
        info["clamped_to_7"] += int((np.abs(unclamped) > 7).sum())
        info["reaches_7"] += int((np.abs(best) == 7).sum())
        info["cut_by_rate"] += int((best != h0).sum())
    return best, best_cost


_LO = np.array([0, 0, -7, -7] * 4 + [-7] * 32, np.int64)
_HI = np.array([7, 7, 0, 0] * 4 + [7] * 32, np.int64)
_BAND = np.arange(BINS) >= 16


def decide(st, lam, info=None):
    """d_stats [n_ctu, 3, 48, 2] -> d_param as uint8 [n_ctu, 3, 8]"""
    st = np.asarray(st, np.int64)
    n_ctu = st.shape[0]
    info = collections.Counter() if info is None else info
    off, cost = offset_search(st[..., 0], st[..., 1], _LO, _HI, lam, _BAND, info)          # [n_ctu, 3, 48]
    j_eo = cost[..., :16].reshape(n_ctu, 3, 4, 4).sum(axis=-1)                            # [n_ctu, 3, 4]
    windows = np.stack([cost[..., 16 + i:16 + i + 29] for i in range(4)]).sum(axis=0)     # [n_ctu, 3, 29]
    pos = windows.argmin(axis=-1)                                                        # the first of equal minima
    j_bo = windows.min(axis=-1)
    info["band_position_tie"] += int(((windows == j_bo[..., None]).sum(axis=-1) > 1).sum())
    out = np.zeros((n_ctu, 3, 8), np.uint8)
    for t in range(n_ctu):
        luma = [lam] + [4 * lam + j_eo[t, 0, k] for k in range(4)] + [7 * lam + j_bo[t, 0]]
        chroma = [lam] + [4 * lam + j_eo[t, 1, k] + j_eo[t, 2, k] for k in range(4)] + [12 * lam + j_bo[t, 1] + j_bo[t, 2]]
        for name, cand, comps in (("luma", luma, (0,)), ("chroma", chroma, (1, 2))):
            pick = int(np.argmin(cand))                                                  # the first of equal minima
            info["tie_to_earlier"] += int(sum(c == cand[pick] for c in cand[pick + 1:]))
            info["%s_%s" % (name, "off" if pick == 0 else "bo" if pick == 5 else "eo%d" % (pick - 1))] += 1
            for m in comps:
                if pick == 0:
                    continue
                typ, arg = (BO, int(pos[t, m])) if pick == 5 else (EO, pick - 1)
                first = 16 + arg if typ == BO else 4 * arg
                out[t, m, 0], out[t, m, 1] = typ, arg
                out[t, m, 2:6] = off[t, m, first:first + 4].astype(np.int8).view(np.uint8)
    return out


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def apply_plane(dec, records, edge):
    """records: uint8 [ctus_y, ctus_x, 8] of this plane's component"""
    p = np.asarray(dec, np.int64)
    ph, pw = p.shape
    cat = categories(p)
    out = p.copy()
    for cy in range(records.shape[0]):
        for cx in range(records.shape[1]):
            rec = records[cy, cx]
            win = (slice(cy * edge, (cy + 1) * edge), slice(cx * edge, (cx + 1) * edge))
            offs = rec[2:6].view(np.int8).astype(np.int64)
            c = p[win]
            if rec[0] == EO:
                table = np.concatenate([[0], offs])
                out[win] = np.clip(c + table[cat[int(rec[1]) & 3][win]], 0, 255)
            elif rec[0] == BO:
                j = ((c >> 3) - int(rec[1])) & 31
                out[win] = np.clip(c + np.where(j < 4, offs[np.minimum(j, 3)], 0), 0, 255)
    return out.astype(np.uint8)


def apply(dec_planes, params, w, h):
    """(y, u, v), d_param [n_ctu, 3, 8] -> the filtered (y, u, v)"""
    nx, ny = ctus(w, h)
    grid = np.asarray(params, np.uint8).reshape(ny, nx, 3, 8)
    return tuple(apply_plane(d, grid[:, :, m], 64 if m == 0 else 32) for m, d in enumerate(dec_planes))


def apply_tiles(oracle, tiles, params, w, h, base):
    """the tile array xSaoApplyGpu leaves: m_Y and m_C filtered from `tiles`, every other byte from `base`"""
    y, u, v = apply(oracle.conv_output_420(tiles, w, h), params, w, h)
    packed = oracle.conv_input_fmt(y, u, v).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    out[:, :384] = packed[:, :384]
    return out.ravel()


def stats_tiles(oracle, org_tiles, dec_tiles, w, h):
    return stats(oracle.conv_output_420(org_tiles, w, h), oracle.conv_output_420(dec_tiles, w, h))


def stats_words(st):
    """[n_ctu, 3, 48, 2] int64 -> the int32 words of d_stats"""
    return np.asarray(st, np.int64).astype(np.int32).ravel()


# ---- the data recipe ------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 64), (80, 48), (144, 80)]
LAMBDAS = (0, 37, 400)
# what happens to CTU t of a case: treatment TREATMENTS[(t + KINDS.index(kind)) % 8], so that a one-CTU frame meets each of them over the
# kinds and a six-CTU frame most of them in every kind
KINDS = ("sharp0", "sharp1", "sharp2", "sharp3", "band", "noise", "far", "same")
TREATMENTS = KINDS


def _blur(p, k):
    """the (1, 2, 1) / 4 blur along EO class k, the plane's border replicated"""
    ph, pw = p.shape
    big = np.pad(p, 1, mode="edge")
    (ax, ay), (bx, by) = NEIGHBOURS[k]
    return (big[1 + ay:1 + ay + ph, 1 + ax:1 + ax + pw] + 2 * p + big[1 + by:1 + by + ph, 1 + bx:1 + bx + pw] + 2) >> 2


def _plane(pw, ph, edge, first, seed):
    """(org, dec) of one plane: org a sinusoid plus +-8 noise (small enough that lambda_q4 = 65535 switches every CTU off); per CTU component
    sharp k  dec = clip8(2 org - blur_k(org)): over-sharpened along class k, which EO class k undoes (a plain blur's errors have the
             sign the EO ranges forbid)
    band     3 subtracted from the samples in 100..131: BO near position 12
    noise    +-1 noise: nothing pays, off
    far      9 added to the samples in 64..95: offsets want -9, the range stops them at -7
    same     dec = org: every cost ties at lambda 0"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    scale = 64 // edge
    r = splitmix64(seed, 0, ph * pw).reshape(ph, pw)
    bits = lambda sh, m: ((r >> np.uint64(sh)) & np.uint64(m)).astype(np.int64)
    org = np.clip(128 + (70 * np.sin(xx * scale / 9.0) * np.cos(yy * scale / 13.0)).astype(np.int64) + bits(8, 31) % 17 - 8, 0, 255)
    dec = org.copy()
    ny, nx = (ph + edge - 1) // edge, (pw + edge - 1) // edge
    for cy in range(ny):
        for cx in range(nx):
            win = (slice(cy * edge, (cy + 1) * edge), slice(cx * edge, (cx + 1) * edge))
            what = TREATMENTS[(cy * nx + cx + first) % len(TREATMENTS)]
            o = org[win]
            if what.startswith("sharp"):
                dec[win] = np.clip(2 * o - _blur(org, int(what[5]))[win], 0, 255)
            elif what == "band":
                dec[win] = np.where((o >= 100) & (o <= 131), o - 3, o)
            elif what == "noise":
                dec[win] = np.clip(o + bits(20, 3)[win] % 3 - 1, 0, 255)
            elif what == "far":
                dec[win] = np.where((o >= 64) & (o <= 95), o + 9, o)
    return org.astype(np.uint8), dec.astype(np.uint8)


def case(kind, w, h):
    """(org planes, dec planes), each (y, u, v) uint8"""
    first = KINDS.index(kind)
    seed = 5000 + 100 * first + w + 3 * h
    pairs = [_plane(w, h, 64, first, seed), _plane(w // 2, h // 2, 32, first, seed + 1), _plane(w // 2, h // 2, 32, first, seed + 2)]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


def squared_error(org, dec, edge):
    """[ctus_y, ctus_x] int64 of one plane"""
    d = (np.asarray(org, np.int64) - np.asarray(dec, np.int64)) ** 2
    ph, pw = d.shape
    ny, nx = (ph + edge - 1) // edge, (pw + edge - 1) // edge
    return np.array([[d[cy * edge:(cy + 1) * edge, cx * edge:(cx + 1) * edge].sum() for cx in range(nx)] for cy in range(ny)], np.int64)
