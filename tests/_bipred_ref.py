"""The reference statement of bi-directional inter prediction (include/x266hip.h: xMotionCompBiQpelTiles, xSatd8x8BiCostsFromTiles,
xSatd8x8RefineBiQpelFromTiles) in numpy int64, and the data recipes of its test cases.  The tables, the vector split and the plane
recipes are tests/_subpel_ref.py's.  For one plane, one reference and one quarter-sample vector

    h(r) = sum_k T[fx][k] S(r, x+ix+k-o)             V = (sum_k T[fy][k] h(y+iy+k-o)) >> 6          (every phase class alike)

and with D = log2_denom + 6

    uni, list l:  clip8(((V_l w_l + (1 << (D - 1))) >> D) + o_l)
    bi:           clip8((V0 w0 + V1 w1 + ((o0 + o1 + 1) << D)) >> (D + 1))
    default:      uni clip8((V + 32) >> 6), bi clip8((V0 + V1 + 64) >> 7)

Nothing here is derived from the library under test."""
import numpy as np

import _subpel_ref as R
from _util import splitmix64

COMP = {"Y": 0, "U": 1, "V": 2}


class WP:
    """x266_wp_t: w, o [list][Y, U, V], log2_denom [luma, chroma]"""

    def __init__(self, w, o, log2_denom):
        self.w, self.o, self.log2_denom = np.array(w, np.int64), np.array(o, np.int64), tuple(int(d) for d in log2_denom)
        assert self.w.shape == (2, 3) and self.o.shape == (2, 3) and len(self.log2_denom) == 2


def V(plane, mv, kind):
    """one plane [ph, pw] uint8, mv [nb, 2] int16 in quarter luma samples per block of that plane -> the intermediate [ph, pw] int64"""
    tab, lg, o, edge = R.PLANE[kind]
    ph, pw = plane.shape
    m = np.asarray(mv, np.int64).reshape(ph // edge, pw // edge, 2)
    ix, fx = R.split(np.repeat(np.repeat(m[..., 0], edge, 0), edge, 1), lg)
    iy, fy = R.split(np.repeat(np.repeat(m[..., 1], edge, 0), edge, 1), lg)
    yy, xx = np.mgrid[0:ph, 0:pw]
    p = np.asarray(plane, np.int64)
    S = lambda y, x: p[np.clip(y, 0, ph - 1), np.clip(x, 0, pw - 1)]
    nt = tab.shape[1]
    tx, ty = tab[fx], tab[fy]
    hsum = lambda r: sum(tx[..., k] * S(r, xx + ix + k - o) for k in range(nt))
    return sum(ty[..., k] * hsum(yy + iy + k - o) for k in range(nt)) >> 6      # numpy's >> on int64 is arithmetic


def combine(v0, v1, direction, wp, comp):
    """the value BEFORE the clip, per sample; direction 1, 2 or 3 (scalar or per sample; 0 gives 0), comp 0, 1, 2 = Y, U, V"""
    v0, v1 = np.asarray(v0, np.int64), np.asarray(v1, np.int64)
    if wp is None:
        uni0, uni1, bi = (v0 + 32) >> 6, (v1 + 32) >> 6, (v0 + v1 + 64) >> 7
    else:
        D = wp.log2_denom[comp != 0] + 6
        w0, w1, o0, o1 = int(wp.w[0, comp]), int(wp.w[1, comp]), int(wp.o[0, comp]), int(wp.o[1, comp])
        uni0 = ((v0 * w0 + (1 << (D - 1))) >> D) + o0
        uni1 = ((v1 * w1 + (1 << (D - 1))) >> D) + o1
        bi = (v0 * w0 + v1 * w1 + ((o0 + o1 + 1) << D)) >> (D + 1)
    d = np.broadcast_to(np.asarray(direction, np.int64) & 3, v0.shape)
    return np.select([d == 1, d == 2, d == 3], [uni0, uni1, bi], 0)


def per_sample(direction, ph, pw, edge):
    """direction [nb] per block (None: all 3) -> [ph, pw]"""
    if direction is None:
        return np.full((ph, pw), 3, np.int64)
    d = np.asarray(direction, np.int64).reshape(ph // edge, pw // edge) & 3
    return np.repeat(np.repeat(d, edge, 0), edge, 1)


def pre_plane(ref0, ref1, mv0, mv1, direction, wp, kind, comp):
    """(values before the clip [ph, pw], direction per sample)"""
    edge = R.PLANE[kind][3]
    d = per_sample(direction, ref0.shape[0], ref0.shape[1], edge)
    return combine(V(ref0, mv0, kind), V(ref1, mv1, kind), d, wp, comp), d


def bi_plane(ref0, ref1, mv0, mv1, direction, wp, kind, comp, base):
    """the predicted plane: blocks of direction 0 keep `base`"""
    pre, d = pre_plane(ref0, ref1, mv0, mv1, direction, wp, kind, comp)
    return np.where(d == 0, base, np.clip(pre, 0, 255)).astype(np.uint8)


def bi_tiles(oracle, ref0_tiles, ref1_tiles, mv0, mv1, direction, wp, w, h, base, planes=3):
    """the tile array xMotionCompBiQpelTiles leaves: m_Y (planes & 1) and / or m_C (planes & 2) predicted, everything else from `base`"""
    p0, p1, pb = (oracle.conv_output_420(t, w, h) for t in (ref0_tiles, ref1_tiles, base))
    py = bi_plane(p0[0], p1[0], mv0, mv1, direction, wp, "luma", 0, pb[0])
    pu = bi_plane(p0[1], p1[1], mv0, mv1, direction, wp, "chroma", 1, pb[1])
    pv = bi_plane(p0[2], p1[2], mv0, mv1, direction, wp, "chroma", 2, pb[2])
    packed = oracle.conv_input_fmt(py, pu, pv).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    if planes & 1:
        out[:, :256] = packed[:, :256]
    if planes & 2:
        out[:, 256:384] = packed[:, 256:384]
    return out.ravel()


def decide(costs, bi_penalty):
    """direction of the least of (c0, c1, c2 + bi_penalty); numpy's argmin returns the first of equal minima"""
    c = np.asarray(costs, np.int64).copy()
    c[:, 2] += int(bi_penalty)
    return (np.argmin(c, axis=1) + 1).astype(np.uint8)


def costs3(oracle, cur_y, ref0_y, ref1_y, mv0, mv1, wp, bi_penalty):
    """(costs [nb, 3] uint32, direction [nb] uint8) of the luma planes"""
    v0, v1 = V(ref0_y, mv0, "luma"), V(ref1_y, mv1, "luma")
    costs = np.stack([R.block_satd(oracle, cur_y, np.clip(combine(v0, v1, d, wp, 0), 0, 255)) for d in (1, 2, 3)], axis=1).astype(np.uint32)
    return costs, decide(costs, bi_penalty)


def refine_bi(oracle, cur_y, fix_y, mv_fix, ref_y, mv_int, lst, wp):
    """49 whole-frame bi predictions -> (mv [nb, 2] int16 in quarter samples, cost [nb] uint32, costs [nb, 49] uint32); `lst` names
    the list being refined, so the candidate's V takes that list's place in the formula"""
    m = np.clip(np.asarray(mv_int, np.int64).reshape(-1, 2), -8191, 8191)
    vf = V(fix_y, mv_fix, "luma")
    costs = np.empty((m.shape[0], 49), np.uint32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            q = 4 * m + np.array([dx, dy], np.int64)
            assert np.abs(q).max() <= 32767
            vc = V(ref_y, q, "luma")
            pre = combine(vc, vf, 3, wp, 0) if lst == 0 else combine(vf, vc, 3, wp, 0)
            costs[:, 7 * (dy + 3) + dx + 3] = R.block_satd(oracle, cur_y, np.clip(pre, 0, 255))
    win = R.winner(costs)
    mv = 4 * m + np.stack([win % 7 - 3, win // 7 - 3], axis=1)
    return mv.astype(np.int16), costs[np.arange(m.shape[0]), win], costs


# ---- data recipes ---------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (32, 32), (64, 64), (48, 32), (144, 80)]
KINDS = R.KINDS
# a negative weight, non-zero offsets, zero and non-zero denominators, and the fields' extremes
WEIGHTS = {
    "fade": WP([[-3, 5, 2], [7, -2, 3]], [[4, -7, 0], [-2, 3, 9]], (2, 1)),
    "denominator 0": WP([[2, 1, -1], [-1, 1, 3]], [[0, 0, 5], [-12, 17, 0]], (0, 0)),
    "field extremes": WP([[127, -128, 127], [127, 127, -128]], [[127, -128, 127], [127, -128, -128]], (0, 7)),
}


def case_planes(kind, w, h):
    """((y, u, v) of list 0, (y, u, v) of list 1) of a size's case"""
    n = KINDS.index(kind)
    return R.planes(kind, w, h, 31 + w + 7 * n), R.planes(kind, w, h, 531 + w + 7 * n)


def unit_weights(d_luma, d_chroma):
    """w = 1 << log2_denom, o = 0: the default, spelled out"""
    return WP([[1 << d_luma, 1 << d_chroma, 1 << d_chroma]] * 2, [[0, 0, 0]] * 2, (d_luma, d_chroma))


def vectors(w, h, seed):
    """(mv0, mv1) of a size's case: list 0 is tests/_subpel_ref.py's recipe (every tap clamps at 16x16, all 16 luma phases at 32x32,
    all 64 chroma phases at 64x64, mv_mix_q otherwise); list 1 is the same set in reversed block order for the enumerated sizes --
    the same phase classes, another vector in every block -- and another mv_mix_q draw otherwise"""
    mv0 = R.vectors(w, h, seed)
    if (w, h) in ((16, 16), (32, 32), (64, 64)):
        return mv0, mv0[::-1].copy()
    return mv0, R.mv_mix_q(len(mv0), w, h, seed + 1000)


def directions(nb, seed):
    """a byte per block whose low two bits take all four values (the first four blocks: 3, 1, 2, 0); the upper six bits are noise,
    which the call must ignore"""
    r = (splitmix64(seed, 0, nb) >> np.uint64(17)).astype(np.uint8)
    r[:4] = (r[:4] & 0xFC) | np.array([3, 1, 2, 0], np.uint8)[:nb]
    return r


def crafted_extremes():
    """two 32x32 planes whose centre sample (16, 16) has V = 33150 and V = -16830 under the vector (2, 2): 255 where TL[2][k] TL[2][j]
    is positive (negative for the second plane) over the 8x8 window of that sample, which both planes tile periodically"""
    t = R.TL[2]
    sign = np.outer(t, t) > 0                                               # [j (rows), k (columns)]: window rows / columns 13..20 of sample 16
    jj, kk = (np.arange(32) - 13) % 8, (np.arange(32) - 13) % 8
    hi = np.where(sign[np.ix_(jj, kk)], 255, 0).astype(np.uint8)
    return hi, (255 - hi).astype(np.uint8)


def decision_case(oracle, w, h, seed):
    """(cur plane, ref0, ref1 planes, mv0, mv1): cur is per block list 0's default prediction, list 1's, or the bi prediction
    (block index mod 3), so with no penalty each of the three directions wins on a share of the blocks"""
    ref0, ref1 = R.plane("random", w, h, seed), R.plane("random", w, h, seed + 1)
    nb = (w // 8) * (h // 8)
    mv0, mv1 = R.mv_mix_q(nb, w, h, seed + 2), R.mv_mix_q(nb, w, h, seed + 3)
    v0, v1 = V(ref0, mv0, "luma"), V(ref1, mv1, "luma")
    src = per_sample(np.arange(nb) % 3 + 1, h, w, 8)
    cur = np.clip(combine(v0, v1, src, None, 0), 0, 255).astype(np.uint8)
    return cur, ref0, ref1, mv0, mv1
