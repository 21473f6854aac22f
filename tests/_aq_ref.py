"""Source analysis of include/x266hip.h (xAqStatsGpu, xAqDecideGpu, xWeightsFromTotals) restated from the header's text: tile records
in numpy uint64 / int64, the qp map in plain loops over CTUs, the fade weights in Python integers.  Also the frames the CPU and the GPU
tests share.  tests/test_aq_ref.py holds it against the values the header states and against exact rational arithmetic."""
import math

import numpy as np

TILE_DTYPE = np.dtype([(name, "<u4") for name in ("sum_y", "ssq_y", "sum_u", "ssq_u", "sum_v", "ssq_v", "energy", "log2_q8")])
assert TILE_DTYPE.itemsize == 32
FIXED_REF_Q8 = 3693
MAX_ENERGY = 6242400
M32 = np.uint64(0xFFFFFFFF)


def log2_q8(e):
    """L(e) of the header, elementwise; the mantissa stays below 2^32 before every squaring, so uint64 holds each product"""
    e = np.maximum(np.asarray(e, np.uint64), np.uint64(1))
    k = np.zeros(e.shape, np.uint64)
    for s in range(1, 32):
        k[(e >> np.uint64(s)) != 0] = s
    m = e << (np.uint64(31) - k)
    f = np.zeros(e.shape, np.uint64)
    for _ in range(8):
        m = (m * m) >> np.uint64(31)
        top = (m >> np.uint64(32)) != 0
        f = (f << np.uint64(1)) | top.astype(np.uint64)
        m = np.where(top, m >> np.uint64(1), m)
    return ((k << np.uint64(8)) | f).astype(np.int64)


def energy(sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v):
    """uint32 arithmetic: every product and difference modulo 2^32"""
    a = [np.asarray(x, np.uint64) for x in (sum_y, ssq_y, sum_u, ssq_u, sum_v, ssq_v)]
    y = (a[1] - (((a[0] * a[0]) & M32) >> np.uint64(8))) & M32
    u = (a[3] - (((a[2] * a[2]) & M32) >> np.uint64(6))) & M32
    v = (a[5] - (((a[4] * a[4]) & M32) >> np.uint64(6))) & M32
    return (y + u + v) & M32


def tile_stats(tiles):
    """the records of a tile array (uint8, 512 bytes per tile): m_Y bytes 0..255, m_C bytes 256..383 (even U, odd V), m_I not read"""
    t = np.ascontiguousarray(tiles, np.uint8).reshape(-1, 512).astype(np.uint64)
    y, u, v = t[:, :256], t[:, 256:384:2], t[:, 257:384:2]
    rec = np.zeros(t.shape[0], TILE_DTYPE)
    for name, plane in (("y", y), ("u", u), ("v", v)):
        rec["sum_" + name] = plane.sum(1)
        rec["ssq_" + name] = (plane * plane).sum(1)
    rec["energy"] = energy(*[rec[n] for n in TILE_DTYPE.names[:6]])
    rec["log2_q8"] = log2_q8(rec["energy"])
    return rec


def totals(rec):
    out = np.zeros(8, np.int64)
    for i, name in enumerate(TILE_DTYPE.names[:6] + ("log2_q8",)):
        out[i] = int(rec[name].astype(np.int64).sum())
    out[7] = rec.size
    return out


def delta(s, n):
    """the mean of n offsets with sum s, rounded to whole qp steps by floor division"""
    return 0 if n == 0 else (2 * s + 256 * n) // (512 * n)


def offsets(rec, total, mode, strength_q8):
    n_tiles = rec.size
    assert mode in (1, 2)
    ref = FIXED_REF_Q8 if mode == 1 else (int(total[6]) + n_tiles // 2) // n_tiles
    return np.clip((strength_q8 * (rec["log2_q8"].astype(np.int64) - ref)) >> 8, -3072, 3072)


def decide(rec, total, w, h, mode, strength_q8, qp, chroma_qp_offset):
    """(Q8 offsets int16 [n_tiles], qp bytes uint8 [6 n_ctu])"""
    tw, th = w // 16, h // 16
    assert rec.size == tw * th
    off = offsets(rec, total, mode, strength_q8)
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
                d = delta(s[q], n[q]) if q < 4 else delta(sum(s), sum(n))
                out[6 * (cy * cw + cx) + q] = min(max(qp + d + (chroma_qp_offset if q >= 4 else 0), 0), 51)
    return off.astype(np.int16), out


def plane_weight(cur, ref, plane, d):
    """(w, o) of plane 0 = Y, 1 = U, 2 = V in Python integers"""
    n = int(cur[7]) * (64 if plane else 256)
    sum_cur, ssq_cur, sum_ref, ssq_ref = int(cur[2 * plane]), int(cur[2 * plane + 1]), int(ref[2 * plane]), int(ref[2 * plane + 1])
    var_cur, var_ref = ssq_cur * n - sum_cur ** 2, ssq_ref * n - sum_ref ** 2
    w = 1 << d if var_ref == 0 else (math.isqrt((var_cur << (2 * d + 2)) // var_ref) + 1) >> 1
    w = min(max(w, 1), 127)
    o = (2 * (sum_cur * (1 << d) - sum_ref * w) + n * (1 << d)) // (2 * n * (1 << d))
    return w, min(max(o, -128), 127)


def weights(cur, ref, log2_denom):
    """([w_y, w_u, w_v], [o_y, o_u, o_v])"""
    pairs = [plane_weight(cur, ref, p, log2_denom[1 if p else 0]) for p in range(3)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def tiles_from_planes(y, u, v, seed=1):
    """a tile array [n_tiles, 512] from planes y [h, w], u and v [h / 2, w / 2]; m_I is seeded garbage that nothing may read"""
    h, w = y.shape
    th, tw = h // 16, w // 16
    t = np.random.RandomState(seed).randint(0, 256, (th * tw, 512)).astype(np.uint8)
    t[:, :256] = np.asarray(y, np.uint8).reshape(th, 16, tw, 16).transpose(0, 2, 1, 3).reshape(-1, 256)
    c = np.stack([np.asarray(u, np.uint8), np.asarray(v, np.uint8)], -1)                     # [h / 2, w / 2, 2]
    t[:, 256:384] = c.reshape(th, 8, tw, 8, 2).transpose(0, 2, 1, 3, 4).reshape(-1, 128)
    return t


def constant_frame(w, h, value):
    return tiles_from_planes(np.full((h, w), value), np.full((h // 2, w // 2), value), np.full((h // 2, w // 2), value))


def max_energy_frame(w, h):
    """every tile: the upper half of each plane 0, the lower half 255"""
    y, c = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8)
    y[np.arange(h) % 16 >= 8] = 255
    c[np.arange(h // 2) % 8 >= 4] = 255
    return tiles_from_planes(y, c, c)


def noise_frame(w, h, seed):
    r = np.random.RandomState(seed)
    return tiles_from_planes(r.randint(0, 256, (h, w)), r.randint(0, 256, (h // 2, w // 2)), r.randint(0, 256, (h // 2, w // 2)), seed + 1)


def halves_frame(w, h, seed):
    """the left half nearly flat (a step of one level), the right half full-range noise: the two modes differ, delta takes both signs"""
    r = np.random.RandomState(seed)
    y, u, v = r.randint(0, 256, (h, w)), r.randint(0, 256, (h // 2, w // 2)), r.randint(0, 256, (h // 2, w // 2))
    half = max(w // 32, 1) * 16
    y[:, :half] = 100 + (np.arange(h)[:, None] // 3 + np.arange(half)[None, :] // 5) % 2
    u[:, :half // 2], v[:, :half // 2] = 90, 160
    return tiles_from_planes(y, u, v, seed + 1)


def distinct_frame(w, h):
    """tile i is the constants (7 i + 3, 11 i + 5, 13 i + 1) mod 256 in Y, U, V: a sample of a neighbour in a sum shows in the record"""
    th, tw = h // 16, w // 16
    i = np.arange(th * tw).reshape(th, tw)
    up = lambda a, k: np.repeat(np.repeat(a, k, 0), k, 1)
    return tiles_from_planes(up((7 * i + 3) % 256, 16), up((11 * i + 5) % 256, 8), up((13 * i + 1) % 256, 8))
