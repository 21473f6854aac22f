"""The reference statement of quarter-sample inter prediction (include/x266hip.h: xMotionCompQpelLumaGpu / ChromaGpu / Gpu and
xSatd8x8RefineQpelFromTilesGpu) in numpy int64 over the planes that oracle.conv_output_420 unpacks, and the data recipes of its
test cases.  For a plane with tap table T, lg phase bits and o taps in front of the sample (luma: TL, 2, 3; chroma: TC, 3, 1):

    ix = mvx >> lg, fx = mvx & (2^lg - 1), iy = mvy >> lg, fy = mvy & (2^lg - 1)         S = the plane with clamped coordinates
    fx = 0, fy = 0:  out = S(y+iy, x+ix)
    fy = 0:          out = clip8((sum_k T[fx][k] S(y+iy, x+ix+k-o) + 32) >> 6)
    fx = 0:          out = clip8((sum_k T[fy][k] S(y+iy+k-o, x+ix) + 32) >> 6)
    otherwise:       h(r) = sum_k T[fx][k] S(r, x+ix+k-o);  v = (sum_k T[fy][k] h(y+iy+k-o)) >> 6;  out = clip8((v + 32) >> 6)

The statement counts what it exercised, per (fx, fy) class.  Nothing here is derived from the library under test."""
import numpy as np

from _util import splitmix64

TL = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)
TC = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
               [-2, 10, 58, -2]], np.int64)
PLANE = {"luma": (TL, 2, 3, 8), "chroma": (TC, 3, 1, 4)}                   # table, lg, o, block edge on that plane


class Counts:
    """per (fx, fy) class: samples, values below 0 and above 255 before the clip, 2-D cases with v < 0"""

    def __init__(self, n):
        self.samples, self.below, self.above, self.negative_v = (np.zeros((n, n), np.int64) for _ in range(4))

    def __iadd__(self, o):
        for k in ("samples", "below", "above", "negative_v"):
            getattr(self, k).__iadd__(getattr(o, k))
        return self

    def __eq__(self, o):
        return all(np.array_equal(getattr(self, k), getattr(o, k)) for k in ("samples", "below", "above", "negative_v"))

    def __repr__(self):
        return "samples %s below %s above %s negative v %s" % tuple(getattr(self, k).tolist() for k in ("samples", "below", "above", "negative_v"))


def split(mv, lg):
    """(integer part, fraction) of a vector component: arithmetic shift, so -1 -> (-1, 2^lg - 1)"""
    mv = np.asarray(mv, np.int64)
    return mv >> lg, mv & ((1 << lg) - 1)


def mc_plane(plane, mv, kind):
    """one plane [ph, pw] uint8, mv [nb, 2] int16 in quarter luma samples, one per block (8x8 on luma, 4x4 on a chroma plane),
    raster order -> (uint8 plane, Counts)"""
    tab, lg, o, edge = PLANE[kind]
    ph, pw = plane.shape
    m = np.asarray(mv, np.int64).reshape(ph // edge, pw // edge, 2)
    ix, fx = split(np.repeat(np.repeat(m[..., 0], edge, 0), edge, 1), lg)
    iy, fy = split(np.repeat(np.repeat(m[..., 1], edge, 0), edge, 1), lg)
    yy, xx = np.mgrid[0:ph, 0:pw]
    p = np.asarray(plane, np.int64)
    S = lambda y, x: p[np.clip(y, 0, ph - 1), np.clip(x, 0, pw - 1)]
    nt = tab.shape[1]
    tx, ty = tab[fx], tab[fy]                                               # [ph, pw, taps]
    hsum = lambda r: sum(tx[..., k] * S(r, xx + ix + k - o) for k in range(nt))
    gather = S(yy + iy, xx + ix)
    hor = (hsum(yy + iy) + 32) >> 6                                         # numpy's >> on int64 is arithmetic
    ver = (sum(ty[..., k] * S(yy + iy + k - o, xx + ix) for k in range(nt)) + 32) >> 6
    v = sum(ty[..., k] * hsum(yy + iy + k - o) for k in range(nt)) >> 6
    both = (v + 32) >> 6
    pre = np.select([(fx == 0) & (fy == 0), fy == 0, fx == 0], [gather, hor, ver], both)
    n = 1 << lg
    c = Counts(n)
    cls = (fx * n + fy).ravel()
    tally = lambda cond: np.bincount(cls[cond.ravel()], minlength=n * n).reshape(n, n)
    c.samples, c.below, c.above = tally(np.ones_like(pre, bool)), tally(pre < 0), tally(pre > 255)
    c.negative_v = tally((fx != 0) & (fy != 0) & (v < 0))
    return np.clip(pre, 0, 255).astype(np.uint8), c


def mc_luma(y, mv):
    return mc_plane(y, mv, "luma")


def mc_chroma(u, v, mv):
    pu, cu = mc_plane(u, mv, "chroma")
    pv, cv = mc_plane(v, mv, "chroma")
    cu += cv
    return pu, pv, cu


def mc_tiles(oracle, ref_tiles, mv, w, h, base, planes="both"):
    """the tile array a call leaves: m_Y and / or m_C predicted from ref_tiles, everything else from `base`"""
    y, u, v = oracle.conv_output_420(ref_tiles, w, h)
    py = mc_luma(y, mv)[0] if planes in ("both", "luma") else y
    pu, pv = mc_chroma(u, v, mv)[:2] if planes in ("both", "chroma") else (u, v)
    packed = oracle.conv_input_fmt(py, pu, pv).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    if planes in ("both", "luma"):
        out[:, :256] = packed[:, :256]
    if planes in ("both", "chroma"):
        out[:, 256:384] = packed[:, 256:384]
    return out.ravel()


def blocks8(plane):
    """[h, w] -> [nb, 64]: the 8x8 blocks in raster order"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def block_satd(oracle, cur_y, pred_y):
    return oracle.satd8x8(blocks8(cur_y.astype(np.int16) - pred_y.astype(np.int16)))


def winner(costs):
    """index 0..48 per block under the tie rule: the centre among equal least costs, after it the first in raster order"""
    costs = np.asarray(costs)
    first = np.argmin(costs, axis=1)                                        # numpy returns the first of equal minima
    return np.where(costs[:, 24] == costs.min(axis=1), 24, first)


def refine(oracle, cur_y, ref_y, mv_int):
    """49 whole-frame predictions -> (mv [nb, 2] int16 in quarter samples, cost [nb] uint32, costs [nb, 49] uint32)"""
    m = np.clip(np.asarray(mv_int, np.int64).reshape(-1, 2), -8191, 8191)
    costs = np.empty((m.shape[0], 49), np.uint32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            q = 4 * m + np.array([dx, dy], np.int64)
            assert np.abs(q).max() <= 32767
            costs[:, 7 * (dy + 3) + dx + 3] = block_satd(oracle, cur_y, mc_luma(ref_y, q)[0])
    win = winner(costs)
    mv = 4 * m + np.stack([win % 7 - 3, win // 7 - 3], axis=1)
    return mv.astype(np.int16), costs[np.arange(m.shape[0]), win], costs


# ---- data recipes ---------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (32, 32), (64, 64), (48, 32), (144, 80), (272, 208)]
KINDS = ("random", "extreme")


def plane(kind, pw, ph, seed):
    """[ph, pw] uint8: "random" 0..255 or "extreme" {0, 255}, the content that reaches both clips"""
    r = splitmix64(seed, 0, ph * pw).reshape(ph, pw)
    if kind == "random":
        return (r & np.uint64(255)).astype(np.uint8)
    return np.where((r >> np.uint64(13)) & np.uint64(1), 255, 0).astype(np.uint8)


def planes(kind, w, h, seed):
    return plane(kind, w, h, seed), plane(kind, w // 2, h // 2, seed + 1), plane(kind, w // 2, h // 2, seed + 2)


def mv_mix_q(nb, w, h, seed):
    """int16 vectors in quarter samples: small ones (-32..31: every luma phase, negative ones too), the int16 extremes, vectors
    pointing wholly outside the frame, and zero"""
    r = splitmix64(seed, 0, 2 * nb).reshape(nb, 2)
    kind = (r >> np.uint64(60)).astype(np.int64)
    small = (r & np.uint64(63)).astype(np.int64) - 32
    ext = np.array([32767, -32768, -32767, 32766], np.int64)[((r >> np.uint64(20)) & np.uint64(3)).astype(np.int64)]
    far = np.where((r >> np.uint64(30)) & np.uint64(1), 1, -1) * (4 * (np.array([w, h], np.int64) + 8) + (r >> np.uint64(40) & np.uint64(255)).astype(np.int64))
    mv = np.select([kind < 8, kind < 11, kind < 14], [small, ext, far], 0)
    return np.clip(mv, -32768, 32767).astype(np.int16)


def vectors(w, h, seed):
    """the vectors of a size's case (see tests/test_gpu_subpel.py)"""
    nb = (w // 8) * (h // 8)
    b = np.arange(nb, dtype=np.int64)
    if (w, h) == (16, 16):                                                  # one tile, every tap clamps: 1-D both ways, 2-D, negative 2-D
        return np.array([[1, 0], [0, 2], [3, 1], [-5, -7]], np.int16)
    if (w, h) == (32, 32):                                                  # luma phase (b & 3, b >> 2): all 16 luma classes
        return np.stack([4 * (b * 5 % 7 - 3) + (b & 3), 4 * (b * 3 % 5 - 2) + (b >> 2)], axis=1).astype(np.int16)
    if (w, h) == (64, 64):                                                  # chroma phase (b & 7, b >> 3): all 64 chroma classes
        return np.stack([8 * (b * 5 % 7 - 3) + (b & 7), 8 * (b * 3 % 5 - 2) + (b >> 3)], axis=1).astype(np.int16)
    return mv_mix_q(nb, w, h, seed)


def _mv_mix(nb, w, h, seed):
    """int16 vectors: small ones (-32..31: all four parity classes, negative odd values), the int16 extremes, vectors pointing
    wholly outside the frame, and zero"""
    r = splitmix64(seed, 0, 2 * nb).reshape(nb, 2)
    kind = (r >> np.uint64(60)).astype(np.int64)
    small = (r & np.uint64(63)).astype(np.int64) - 32
    ext = np.array([32767, -32768, -32767, 32766], np.int64)[((r >> np.uint64(20)) & np.uint64(3)).astype(np.int64)]
    far = np.where((r >> np.uint64(30)) & np.uint64(1), 1, -1) * (np.array([w, h], np.int64) + 8 + (r >> np.uint64(40) & np.uint64(255)).astype(np.int64))
    mv = np.select([kind < 8, kind < 11, kind < 14], [small, ext, far], 0)
    return np.clip(mv, -32768, 32767).astype(np.int16)
