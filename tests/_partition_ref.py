"""The reference statement of the inter partition decision (include/x266hip.h, "inter partition decision": xInterPartitionDecideGpu) in
numpy and Python integers over luma planes, and the data recipes of its test cases.  With bw = w / 8, bh = h / 8 and n = 1 << k:

    in(bx, by)      clamp(component, -32766, 32766) of the input field
    D(b, q)         satd8x8(cur_b - P_q(b)), P_q the luma prediction of xMotionCompQpelLumaGpu under q (_subpel_ref.mc_luma)
    predictor       A = in(X - 1, Y), B = in(X, Y - 1), C = in(X + n, Y - 1) if inside the frame else in(X - 1, Y - 1); exactly one inside:
                    that one; otherwise the component-wise median, a block outside counting as (0, 0)
    R(k, q)         (k > 0) + L(qx - Px) + L(qy - Py), L of _seeded_ref.code_length;  Jw = D(node, q) + ((lambda_q4 * R) >> 4)
    winners         W(b) = in(b); a whole node walks its children TL, TR, BL, BR, per child dy = -r..r, then dx = -r..r:
                    q = clamp16(W(child) + (dx, dy)); the least Jw, the first of equal ones
    decision        Best(b) = Jw(b, W(b)); whole node: S = sum Best(children) + (lambda_q4 >> 4), one partition if Jw(W) <= S, else Best = S;
                    cut node: the sum over its existing children, no flag

The walk is brute force in exactly that order.  The prediction of a node under a vector is mc_luma on a crop of the reference gathered
with clamped coordinates, wide enough that no tap leaves it, so every sample is _subpel_ref's; every SATD comes from the oracle.
Nothing here is derived from the library under test."""
import numpy as np

import _seeded_ref as S
import _subpel_ref as Q
from _util import splitmix64

ME_DTYPE = S.ME_DTYPE
CTU_DTYPE = np.dtype([("j", "<u4"), ("dist", "<u4"), ("bits", "<u4"), ("parts", "<u4")])
CLAMP = 32766
LEVELS = 4


def clamp_in(c):
    return max(-CLAMP, min(CLAMP, int(c)))


def clamp16(c):
    return max(-32768, min(32767, int(c)))


def field_in(mv, w, h):
    """in() of the whole field: [bh, bw, 2] int64"""
    return np.clip(np.asarray(mv, np.int64).reshape(h // 8, w // 8, 2), -CLAMP, CLAMP)


def whole(bw, bh, k, nx, ny):
    return nx < (bw >> k) and ny < (bh >> k)


def exists(bw, bh, k, nx, ny):
    return (nx << k) < bw and (ny << k) < bh


def nodes_offset(bw, bh, k):
    """the first d_nodes record of level k: level 1 first, then 2, then 3"""
    return sum((bw >> j) * (bh >> j) for j in range(1, k))


def nodes_total(bw, bh):
    return nodes_offset(bw, bh, LEVELS)


def median3(a, b, c):
    return sorted((a, b, c))[1]


def predictor(fin, X, Y, n):
    """P of the node of n blocks a side at block (X, Y); fin = field_in(...)"""
    bh, bw = fin.shape[:2]
    inside = lambda x, y: 0 <= x < bw and 0 <= y < bh
    at = lambda x, y: (int(fin[y, x, 0]), int(fin[y, x, 1]))
    spots = [(X - 1, Y), (X, Y - 1), (X + n, Y - 1) if inside(X + n, Y - 1) else (X - 1, Y - 1)]
    have = [at(*p) for p in spots if inside(*p)]
    if len(have) == 1:
        return have[0]
    three = [at(*p) if inside(*p) else (0, 0) for p in spots]
    return median3(*(v[0] for v in three)), median3(*(v[1] for v in three))


def rate(k, q, p):
    return (1 if k > 0 else 0) + S.code_length(q[0] - p[0]) + S.code_length(q[1] - p[1])


def rate_cost(lam, bits):
    return (int(lam) * int(bits)) >> 4


def walk(children, r):
    """the candidates of a node whose children's winners are `children` (TL, TR, BL, BR), in the order they are tried"""
    return [(clamp16(cx + dx), clamp16(cy + dy)) for cx, cy in children for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


class Distortion:
    """D(b, q) for the blocks of a node, [n, n] int64, cached per (X, Y, n, q)"""
    MARGIN = 4                                                              # samples around the node: the taps reach 3 before, 4 behind

    def __init__(self, oracle, cur_y, ref_y):
        self.oracle, self.cur, self.ref = oracle, np.asarray(cur_y), np.asarray(ref_y)
        self.cache = {}

    def many(self, X, Y, n, qs):
        """[D(node, q) per q of qs]: the vectors not yet cached go through ONE mc_luma and one SATD call, their crops side by side in one
        plane (a crop's margin keeps every tap of its node inside it)"""
        todo = [q for q in dict.fromkeys(qs) if (X, Y, n, q) not in self.cache]
        if todo:
            h, w = self.ref.shape
            side, m = 8 * n, self.MARGIN
            full = side + 2 * m
            crops, fracs = [], []
            for q in todo:
                ys = np.clip(8 * Y + (q[1] >> 2) - m + np.arange(full), 0, h - 1)
                xs = np.clip(8 * X + (q[0] >> 2) - m + np.arange(full), 0, w - 1)
                crops.append(self.ref[ys[:, None], xs[None, :]])
                fracs.append(np.tile(np.array([[[q[0] & 3, q[1] & 3]]], np.int16), (full // 8, full // 8, 1)))
            pred = Q.mc_luma(np.concatenate(crops, axis=1), np.concatenate(fracs, axis=1).reshape(-1, 2))[0]
            pred = pred.reshape(full, len(todo), full)[m:m + side, :, m:m + side].astype(np.int16)
            cur = self.cur[8 * Y:8 * Y + side, 8 * X:8 * X + side].astype(np.int16)
            diff = (cur[:, None, :] - pred).reshape(side, len(todo) * side)
            d = np.asarray(self.oracle.satd8x8(Q.blocks8(diff)), np.int64).reshape(n, len(todo), n)
            for i, q in enumerate(todo):
                self.cache[X, Y, n, q] = d[:, i, :]
        return [self.cache[X, Y, n, q] for q in qs]

    def __call__(self, X, Y, n, q):
        return self.many(X, Y, n, [q])[0]


def decide(oracle, cur_y, ref_y, mv, r, lam):
    """-> dict: out [nb] ME_DTYPE, level [nb] uint8, ctu [n_ctu] CTU_DTYPE, nodes [nodes_total] ME_DTYPE (W and Jw of the whole nodes),
    merged {(k, nx, ny): bool} of the whole nodes of levels 1..3, cut_split: the cut nodes (all of them split)"""
    h, w = cur_y.shape
    bw, bh = w // 8, h // 8
    fin = field_in(mv, w, h)
    D = Distortion(oracle, cur_y, ref_y)
    W, JW, DW, RW = {}, {}, {}, {}                                          # per whole node: winner, its Jw, its per-block D, its R
    d0 = Q.block_satd(oracle, cur_y, Q.mc_luma(ref_y, fin.reshape(-1, 2))[0]).astype(np.int64)    # level 0: the field itself, one prediction
    for by in range(bh):
        for bx in range(bw):
            q = (int(fin[by, bx, 0]), int(fin[by, bx, 1]))
            W[0, bx, by], DW[0, bx, by] = q, d0[by * bw + bx].reshape(1, 1)
            RW[0, bx, by] = rate(0, q, predictor(fin, bx, by, 1))
            JW[0, bx, by] = int(DW[0, bx, by].sum()) + rate_cost(lam, RW[0, bx, by])
    nodes = np.zeros(nodes_total(bw, bh), ME_DTYPE)
    for k in range(1, LEVELS):
        n = 1 << k
        for ny in range(bh >> k):
            for nx in range(bw >> k):
                X, Y = nx << k, ny << k
                p = predictor(fin, X, Y, n)
                best = None
                cands = walk([W[k - 1, 2 * nx + (c & 1), 2 * ny + (c >> 1)] for c in range(4)], r)
                for q, d in zip(cands, D.many(X, Y, n, cands)):
                    bits = rate(k, q, p)
                    j = int(d.sum()) + rate_cost(lam, bits)
                    if best is None or j < best[0]:                         # the first of equal ones stays
                        best = (j, q, bits)
                assert best[0] < 1 << 32
                JW[k, nx, ny], W[k, nx, ny], RW[k, nx, ny] = best
                DW[k, nx, ny] = D(X, Y, n, best[1])
                nodes[nodes_offset(bw, bh, k) + ny * (bw >> k) + nx] = (best[1][0], best[1][1], best[0])
    merged, cut_split, best_of = {}, [], {}

    def settle(k, nx, ny):
        """Best of the node -> (j, dist, bits, parts); fills merged / cut_split on the way"""
        if k == 0:
            best_of[k, nx, ny] = (JW[0, nx, ny], int(DW[0, nx, ny].sum()), RW[0, nx, ny], 1)
            return best_of[k, nx, ny]
        kids = [settle(k - 1, 2 * nx + (c & 1), 2 * ny + (c >> 1)) for c in range(4) if exists(bw, bh, k - 1, 2 * nx + (c & 1), 2 * ny + (c >> 1))]
        j, dist, bits, parts = (sum(v[i] for v in kids) for i in range(4))
        if whole(bw, bh, k, nx, ny):
            split = j + rate_cost(lam, 1)
            merged[k, nx, ny] = JW[k, nx, ny] <= split                      # a tie merges
            res = (JW[k, nx, ny], int(DW[k, nx, ny].sum()), RW[k, nx, ny], 1) if merged[k, nx, ny] else (split, dist, bits + 1, parts)
        else:
            cut_split.append((k, nx, ny))
            res = (j, dist, bits, parts)
        best_of[k, nx, ny] = res
        return res

    cw, ch = (w + 63) // 64, (h + 63) // 64
    ctu = np.zeros(cw * ch, CTU_DTYPE)
    for cy in range(ch):
        for cx in range(cw):
            ctu[cy * cw + cx] = settle(3, cx, cy)
    out, level = np.zeros(bw * bh, ME_DTYPE), np.zeros(bw * bh, np.uint8)
    for by in range(bh):
        for bx in range(bw):
            k = max([0] + [j for j in range(1, LEVELS) if merged.get((j, bx >> j, by >> j))])
            node = (k, bx >> k, by >> k)
            out[by * bw + bx] = (W[node][0], W[node][1], DW[node][by - ((by >> k) << k), bx - ((bx >> k) << k)])
            level[by * bw + bx] = k
    return dict(out=out, level=level, ctu=ctu, nodes=nodes, merged=merged, cut_split=cut_split, jw0=np.array([JW[0, b % bw, b // bw] for b in range(bw * bh)]),
                d0=np.array([int(DW[0, b % bw, b // bw].sum()) for b in range(bw * bh)]))


def ctu_of_block(w, b):
    bw = w // 8
    return ((b // bw) >> 3) * ((w + 63) // 64) + ((b % bw) >> 3)


# ---- data recipes -----------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (64, 64), (80, 48), (144, 112), (1104, 16)]
SETTINGS = [(0, 0), (64, 1), (4096, 1), (65535, 0)]                        # (lambda_q4, range)


def motion_map(w, h):
    """whole-sample motion per sample, [h, w, 2] (x, y): two regions split by a slanted line and a 24 x 24 patch with a third motion"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w, 2), np.int64)
    left = xx + yy // 4 < (5 * w) // 8
    m[left] = (2, -1)
    m[~left] = (-6, 4)
    py, px = min(40, max(h - 24, 0) // 8 * 8), min(72, max(w - 24, 0) // 8 * 8)
    m[py:py + 24, px:px + 24] = (9, -7)
    return m


def motion_frames(w, h, seed):
    """(cur, ref) luma planes: a smoothed texture, cur = ref moved by motion_map, +-2 noise"""
    ref = S.smooth_texture(w, h, 0xA11CE + seed)
    m = motion_map(w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    moved = ref[np.clip(yy + m[..., 1], 0, h - 1), np.clip(xx + m[..., 0], 0, w - 1)].astype(np.int64)
    noise = (splitmix64(0xB0B + seed, 0, w * h) % np.uint64(5)).astype(np.int64).reshape(h, w) - 2
    return np.clip(moved + noise, 0, 255).astype(np.uint8), ref


def motion_field(w, h, seed):
    """the per-block vector of that motion (the motion at the block's centre) in quarter samples, jittered by -1, 0 or 1: [nb, 2] int16"""
    m = motion_map(w, h)[4::8, 4::8].reshape(-1, 2) * 4
    jitter = (splitmix64(0xD1CE + seed, 0, m.size) % np.uint64(3)).astype(np.int64).reshape(-1, 2) - 1
    return (m + jitter).astype(np.int16)


def mix_frames(w, h, seed):
    """random content for the vector mix of _subpel_ref.mv_mix_q: the clamps and the far-outside vectors"""
    return Q.plane("random", w, h, 0x51DE + seed), Q.plane("random", w, h, 0x52DE + seed)


def mix_field(w, h, seed):
    return Q.mv_mix_q((w // 8) * (h // 8), w, h, 0x53DE + seed)
