"""The reference statement of in-loop deblocking (include/x266hip.h: xDeblockLumaGpu / ChromaGpu / Gpu) in numpy int64 over the
planes that oracle.conv_output_420 unpacks, and the data recipes of its test cases.  Whole-frame: per plane all vertical edges,
then all horizontal edges on the result (the horizontal pass is the vertical one on the transposed plane).  The statement counts
what it exercised, per plane and edge direction.  Nothing here is derived from the library under test.

Luma, per 8-sample edge between the 8x8 blocks P and Q:  transform edge = different luma regions, or the coordinate is a multiple
of the region's N = 4 << (class & 3);  Bs = 2 (transform edge, an intra side), 1 (transform edge, a coded side), 1 (no intra side,
vectors differ by >= 4 in a component), else 0;  qP = (qpP + qpQ + 1) >> 1, beta = BETA[clamp(qP + 2 bo, 0, 51)],
tc = TC[clamp(qP + 2 (Bs - 1) + 2 to, 0, 53)];  per 4-line segment the decisions d < beta, strong, dEp, dEq from lines 0 and 3;
the strong or the normal filter per line.  Chroma, per plane and tile boundary: filtered iff transform edge of that plane's region
and an intra luma quadrant on either side; tc = TC[clamp(qPc + 2 + 2 to, 0, 53)]; D = clamp((((q0 - p0) << 2) + p1 - q1 + 4) >> 3, -tc, tc)."""
import collections

import numpy as np

from _util import splitmix64

BETA = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 65, 2)), np.int64)
TC = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5] * 2 + [6] * 2 + [7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], np.int64)
assert BETA.size == 52 and TC.size == 54

PASSES = ("luma_v", "luma_h", "u_v", "u_h", "v_v", "v_h")


def new_counts():
    return {k: collections.Counter() for k in PASSES}


def add_counts(total, more):
    for k in PASSES:
        total[k].update(more[k])
    return total


class Side:
    """the side information of a call: cls, intra, qps uint8 [n_ctu, 6], nnz uint32 [n_ctu, 6], mv int16 [nb, 2] -- or None, the
    header's default for that array -- and the three scalars"""

    def __init__(self, cls=None, intra=None, nnz=None, qps=None, mv=None, qp=0, beta_offset_div2=0, tc_offset_div2=0):
        self.cls, self.intra, self.nnz, self.qps, self.mv = cls, intra, nnz, qps, mv
        self.qp, self.beta_offset_div2, self.tc_offset_div2 = qp, beta_offset_div2, tc_offset_div2

    def kwargs(self):
        return dict(cls=self.cls, intra=self.intra, nnz=self.nnz, qps=self.qps, mv=self.mv, qp=self.qp,
                    beta_offset_div2=self.beta_offset_div2, tc_offset_div2=self.tc_offset_div2)

    def replace(self, **kw):
        d = self.kwargs()
        d.update(kw)
        return Side(**d)

    # per region index r = 6 ctu + q (arrays of any shape)
    def n(self, r):
        return np.full(np.shape(r), 32, np.int64) if self.cls is None else 4 << (np.asarray(self.cls, np.int64).ravel()[r] & 3)

    def is_intra(self, r):
        return np.zeros(np.shape(r), bool) if self.intra is None else np.asarray(self.intra).ravel()[r] != 0

    def coded(self, r):
        return np.ones(np.shape(r), bool) if self.nnz is None else np.asarray(self.nnz).ravel()[r] != 0

    def region_qp(self, r):
        return np.full(np.shape(r), self.qp, np.int64) if self.qps is None else np.minimum(np.asarray(self.qps, np.int64).ravel()[r], 51)


def ctus(w, h):
    return (w + 63) // 64, (h + 63) // 64


# ---- parameters of all edges of one direction ----------------------------------------------------------------------------------------
def luma_edges(side, w, h, vertical, c):
    """(bs, beta, tc), each [h/8, w/8 - 1] for vertical edges ([by, k - 1]: the edge at x = 8k) or [h/8 - 1, w/8] for horizontal ones"""
    cx = ctus(w, h)[0]
    by, bx = np.mgrid[0:h // 8, 0:w // 8]
    if vertical:
        (pbx, pby), (qbx, qby) = (bx[:, :-1], by[:, :-1]), (bx[:, 1:], by[:, 1:])
        coord = 8 * qbx
    else:
        (pbx, pby), (qbx, qby) = (bx[:-1], by[:-1]), (bx[1:], by[1:])
        coord = 8 * qby
    region = lambda x, y: ((y >> 3) * cx + (x >> 3)) * 6 + ((y >> 2) & 1) * 2 + ((x >> 2) & 1)
    rp, rq = region(pbx, pby), region(qbx, qby)
    n = side.n(rq)
    tr = (rp != rq) | (coord % n == 0)
    intra = side.is_intra(rp) | side.is_intra(rq)
    coded = side.coded(rp) | side.coded(rq)
    motion = np.zeros(tr.shape, bool)
    if side.mv is not None:
        m = np.asarray(side.mv, np.int64).reshape(h // 8, w // 8, 2)
        motion = (np.abs(m[pby, pbx] - m[qby, qbx]) >= 4).any(axis=-1)
    rule = np.select([tr & intra, tr & coded, ~intra & motion], [1, 2, 3], 0)
    bs = np.array([0, 2, 1, 1], np.int64)[rule]
    qpp, qpq = side.region_qp(rp), side.region_qp(rq)
    qp = (qpp + qpq + 1) >> 1
    bi, ti = qp + 2 * side.beta_offset_div2, qp + 2 * (bs - 1) + 2 * side.tc_offset_div2
    on = bs > 0
    for name, r in (("rule_intra", 1), ("rule_coded", 2), ("rule_motion", 3)):
        c[name] += 2 * int((rule == r).sum())                              # two segments per edge
    for k in (0, 1, 2):
        c["bs%d" % k] += 2 * int((bs == k).sum())
    for size in (4, 8, 16, 32):
        c["edges_n%d" % size] += int((n == size).sum())
        c["transform_n%d" % size] += int((tr & (n == size)).sum())
    c["not_transform"] += int((~tr).sum())
    c["qp_differs"] += int((on & (qpp != qpq)).sum())
    c["beta_index_below_0"] += int((on & (bi < 0)).sum())
    c["beta_index_above_51"] += int((on & (bi > 51)).sum())
    c["tc_index_below_0"] += int((on & (ti < 0)).sum())
    c["tc_index_above_53"] += int((on & (ti > 53)).sum())
    return bs, BETA[np.clip(bi, 0, 51)], TC[np.clip(ti, 0, 53)]


def chroma_edges(side, w, h, plane, vertical, c):
    """(filtered, tc), each [h/16, w/16 - 1] (vertical) or [h/16 - 1, w/16] (horizontal); plane 0 = U, 1 = V"""
    cx = ctus(w, h)[0]
    ty, tx = np.mgrid[0:h // 16, 0:w // 16]
    if vertical:
        (ptx, pty), (qtx, qty) = (tx[:, :-1], ty[:, :-1]), (tx[:, 1:], ty[:, 1:])
        coord = 8 * qtx
    else:
        (ptx, pty), (qtx, qty) = (tx[:-1], ty[:-1]), (tx[1:], ty[1:])
        coord = 8 * qty
    ctu = lambda x, y: (y >> 2) * cx + (x >> 2)
    quad = lambda x, y: ctu(x, y) * 6 + ((y >> 1) & 1) * 2 + ((x >> 1) & 1)
    cp, cq = ctu(ptx, pty), ctu(qtx, qty)
    n = side.n(cq * 6 + 4 + plane)
    tr = (cp != cq) | (coord % n == 0)
    intra = side.is_intra(quad(ptx, pty)) | side.is_intra(quad(qtx, qty))
    qpp, qpq = side.region_qp(cp * 6 + 4 + plane), side.region_qp(cq * 6 + 4 + plane)
    ti = ((qpp + qpq + 1) >> 1) + 2 + 2 * side.tc_offset_div2
    on = tr & intra
    c["filtered"] += int(on.sum())
    c["not_transform"] += int((~tr).sum())
    c["not_intra"] += int((tr & ~intra).sum())
    for size in (4, 8, 16, 32):
        c["edges_n%d" % size] += int((n == size).sum())
        c["transform_n%d" % size] += int((tr & (n == size)).sum())
    c["qp_differs"] += int((on & (qpp != qpq)).sum())
    c["tc_index_below_0"] += int((on & (ti < 0)).sum())
    c["tc_index_above_53"] += int((on & (ti > 53)).sum())
    return on, TC[np.clip(ti, 0, 53)]


# ---- the vertical passes (the horizontal ones are these on the transposed plane) ---------------------------------------------------------
def luma_vertical(p, bs, beta, tc, c):
    """p: int64 [rows, cols], changed in place; bs, beta, tc: [rows / 8, cols / 8 - 1]"""
    rows, cols = p.shape
    k = cols // 8 - 1
    if k == 0:
        return
    idx = 8 * (np.arange(k)[:, None] + 1) - 4 + np.arange(8)[None, :]       # [k, 8]: p3 p2 p1 p0 q0 q1 q2 q3
    a = p[:, idx]                                                           # [rows, k, 8]
    seg = lambda x: np.repeat(x, 2, axis=0)                                 # per edge -> per segment
    line = lambda x: np.repeat(x, 4, axis=0)                                # per segment -> per line
    bs_s, beta_s, tc_s = seg(bs), seg(beta), seg(tc)
    a4 = a.reshape(rows // 4, 4, k, 8)
    dpi = [np.abs(l[..., 1] - 2 * l[..., 2] + l[..., 3]) for l in (a4[:, 0], a4[:, 3])]
    dqi = [np.abs(l[..., 6] - 2 * l[..., 5] + l[..., 4]) for l in (a4[:, 0], a4[:, 3])]
    dp, dq = dpi[0] + dpi[1], dqi[0] + dqi[1]
    on = (bs_s > 0) & (dp + dq < beta_s)
    strong = on.copy()
    for i, l in enumerate((a4[:, 0], a4[:, 3])):
        strong &= (2 * (dpi[i] + dqi[i]) < (beta_s >> 2)) & (np.abs(l[..., 0] - l[..., 3]) + np.abs(l[..., 4] - l[..., 7]) < (beta_s >> 3)) & \
                  (np.abs(l[..., 3] - l[..., 4]) < ((5 * tc_s + 1) >> 1))
    side_thr = (beta_s + (beta_s >> 1)) >> 3
    dep, deq = dp < side_thr, dq < side_thr
    c["seg_off"] += int(((bs_s > 0) & ~on).sum())
    c["seg_strong"] += int(strong.sum())
    c["seg_normal"] += int((on & ~strong).sum())
    on_l, strong_l, dep_l, deq_l, tc_l = line(on), line(strong), line(dep), line(deq), line(tc_s)
    p3, p2, p1, p0, q0, q1, q2, q3 = (a[..., i] for i in range(8))
    out = a.copy()
    # strong
    t2 = 2 * tc_l
    raw = {3: (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, 2: (p2 + p1 + p0 + q0 + 2) >> 2, 1: (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3,
           4: (q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3, 5: (q2 + q1 + q0 + p0 + 2) >> 2, 6: (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3}
    clamped = np.zeros(on_l.shape, bool)
    for i, v in raw.items():
        lim = np.clip(v, a[..., i] - t2, a[..., i] + t2)
        clamped |= strong_l & (lim != v)
        out[..., i] = np.where(strong_l, lim, out[..., i])
    c["clamp_2tc"] += int(clamped.sum())
    # normal
    normal = on_l & ~strong_l
    delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
    skip = normal & (np.abs(delta) >= 10 * tc_l)
    run = normal & ~skip
    c["line_skip"] += int(skip.sum())
    for ep in (0, 1):
        for eq in (0, 1):
            c["normal_ep%d_eq%d" % (ep, eq)] += int((run & (dep_l == bool(ep)) & (deq_l == bool(eq))).sum())
    d = np.clip(delta, -tc_l, tc_l)
    c["clamp_tc"] += int((run & (d != delta)).sum())
    h = tc_l >> 1
    new = {3: p0 + d, 4: q0 - d, 2: p1 + np.clip((((p2 + p0 + 1) >> 1) - p1 + d) >> 1, -h, h), 5: q1 + np.clip((((q2 + q0 + 1) >> 1) - q1 - d) >> 1, -h, h)}
    use = {3: run, 4: run, 2: run & dep_l, 5: run & deq_l}
    clipped = np.zeros(on_l.shape, bool)
    for i, v in new.items():
        clipped |= use[i] & ((v < 0) | (v > 255))
        out[..., i] = np.where(use[i], np.clip(v, 0, 255), out[..., i])
    c["clip8"] += int(clipped.sum())
    p[:, idx] = out


def chroma_vertical(p, on, tc, c):
    """p: int64 [rows, cols] of one chroma plane, changed in place; on, tc: [rows / 8, cols / 8 - 1]"""
    rows, cols = p.shape
    k = cols // 8 - 1
    if k == 0:
        return
    idx = 8 * (np.arange(k)[:, None] + 1) - 2 + np.arange(4)[None, :]       # p1 p0 q0 q1
    a = p[:, idx]
    on_l, tc_l = np.repeat(on, 8, axis=0), np.repeat(tc, 8, axis=0)
    p1, p0, q0, q1 = (a[..., i] for i in range(4))
    raw = (((q0 - p0) << 2) + p1 - q1 + 4) >> 3
    d = np.clip(raw, -tc_l, tc_l)
    c["lines"] += int(on_l.sum())
    c["clamp_tc"] += int((on_l & (d != raw)).sum())
    c["clip8"] += int((on_l & ((p0 + d < 0) | (p0 + d > 255) | (q0 - d < 0) | (q0 - d > 255))).sum())
    out = a.copy()
    out[..., 1] = np.where(on_l, np.clip(p0 + d, 0, 255), p0)
    out[..., 2] = np.where(on_l, np.clip(q0 - d, 0, 255), q0)
    p[:, idx] = out


# ---- whole planes -------------------------------------------------------------------------------------------------------------------------
def deblock_luma(y, side, counts=None):
    counts = new_counts() if counts is None else counts
    h, w = y.shape
    p = np.array(y, np.int64)
    luma_vertical(p, *luma_edges(side, w, h, True, counts["luma_v"]), counts["luma_v"])
    t = np.ascontiguousarray(p.T)
    luma_vertical(t, *(x.T for x in luma_edges(side, w, h, False, counts["luma_h"])), counts["luma_h"])
    return t.T.astype(np.uint8), counts


def deblock_chroma(u, v, side, counts=None):
    counts = new_counts() if counts is None else counts
    out = []
    for plane, (name, src) in enumerate((("u", u), ("v", v))):
        ch, cw = src.shape
        p = np.array(src, np.int64)
        chroma_vertical(p, *chroma_edges(side, 2 * cw, 2 * ch, plane, True, counts[name + "_v"]), counts[name + "_v"])
        t = np.ascontiguousarray(p.T)
        chroma_vertical(t, *(x.T for x in chroma_edges(side, 2 * cw, 2 * ch, plane, False, counts[name + "_h"])), counts[name + "_h"])
        out.append(t.T.astype(np.uint8))
    return out[0], out[1], counts


def deblock_tiles(oracle, tiles, w, h, side, base=None, planes="both", counts=None):
    """the tile array a call leaves: m_Y and / or m_C deblocked from `tiles`, everything else from `base` (None: from `tiles`, the
    in-place case)"""
    y, u, v = oracle.conv_output_420(tiles, w, h)
    py = deblock_luma(y, side, counts)[0] if planes in ("both", "luma") else y
    pu, pv = deblock_chroma(u, v, side, counts)[:2] if planes in ("both", "chroma") else (u, v)
    packed = oracle.conv_input_fmt(py, pu, pv).reshape(-1, 512)
    out = np.array(tiles if base is None else base, np.uint8).reshape(-1, 512)
    if planes in ("both", "luma"):
        out[:, :256] = packed[:, :256]
    if planes in ("both", "chroma"):
        out[:, 256:384] = packed[:, 256:384]
    return out.ravel()


# ---- data recipes -------------------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (32, 32), (64, 64), (80, 48)]
COMPOSITE = [(144, 80), (272, 208)]
KINDS = ("blocks", "smooth", "steps", "extreme", "constant", "profile")
# (beta_offset_div2, tc_offset_div2) of a kind's case: the neutral pair, both ends, and two mixed ones
OFFSETS = {"blocks": (0, 0), "smooth": (6, 6), "steps": (-2, 3), "extreme": (3, -1), "constant": (-6, -6), "profile": (6, -6)}
# per sample position modulo 8 (q0 q1 q2 q3 p3 p2 p1 p0 of the edges on either side): flat enough for the strong filter at beta >= 48, and
# with tc = 1 its p0' = (6 + 6 + 0 + 4 + 4 + 4) >> 3 = 3 lies outside p0 +- 2 tc -- the clamp that smooth content never reaches
PROFILE = np.array([2, 4, 6, 2, 5, 6, 3, 0], np.int64)


def _rand(seed, n):
    return splitmix64(seed, 0, n)


def plane(kind, pw, ph, seed):
    """[ph, pw] uint8.  Uniform noise almost never passes d < beta, so the content is built from per-8x8-block levels:
    "blocks"  levels 128 +- 24, a gentle ramp and +-2 noise: normal filtering with every (dEp, dEq) combination
    "smooth"  levels that differ by a few units, no noise: the strong filter
    "steps"   levels anywhere in 16..239 with +-1 noise: large steps, lines skipped by |D| >= 10 tc, segments switched off
    "extreme" levels 0 or 255 with noise folded back into 0..255: clip8
    "constant" one value
    "profile" PROFILE[x & 7] + PROFILE[y & 7] on one level: the strong filter's +-2 tc clamp, in both passes (the filters commute with
              adding a constant, so the rows still differ by constants after the vertical pass)"""
    r = _rand(seed, ph * pw).reshape(ph, pw)
    rb = np.repeat(np.repeat(_rand(seed + 1000, (ph // 8) * (pw // 8)).reshape(ph // 8, pw // 8), 8, 0), 8, 1)
    yy, xx = np.mgrid[0:ph, 0:pw]
    bits = lambda a, sh, m: ((a >> np.uint64(sh)) & np.uint64(m)).astype(np.int64)
    if kind == "blocks":
        v = 104 + bits(rb, 8, 63) * 3 // 4 + (xx + 2 * yy) // 8 + bits(r, 3, 7) % 5 - 2
    elif kind == "smooth":
        v = 120 + bits(rb, 8, 7) + (xx + yy) // 16
    elif kind == "steps":
        v = 16 + bits(rb, 8, 255) * 7 // 8 + bits(r, 5, 3) % 3 - 1
    elif kind == "extreme":
        high = bits(rb, 8, 3) != 0
        v = np.where(high, 255, 0) + np.where(high, -1, 1) * ((4 + bits(r, 4, 3)) * bits(r, 9, 1))
    elif kind == "profile":
        v = 100 + PROFILE[xx & 7] + PROFILE[yy & 7]
    else:
        v = np.full((ph, pw), 77 + seed % 100, np.int64)
    return np.clip(v, 0, 255).astype(np.uint8)


def planes(kind, w, h, seed):
    return plane(kind, w, h, seed), plane(kind, w // 2, h // 2, seed + 1), plane(kind, w // 2, h // 2, seed + 2)


def side_mix(kind, w, h, seed):
    """mixed classes per region (with type bits above the size bits, which the filter must ignore), a mixed intra / coded / qp
    pattern (qp bytes up to 63: the clamp to 51) and mixed vectors: mostly shared between neighbours, some differing by less than
    4, some by more, some at the int16 extremes (their difference needs more than 16 bits)"""
    n = ctus(w, h)[0] * ctus(w, h)[1] * 6
    nb = (w // 8) * (h // 8)
    bits = lambda a, sh, m: ((a >> np.uint64(sh)) & np.uint64(m)).astype(np.int64)
    k = KINDS.index(kind)
    r = _rand(seed, n)
    q = np.arange(n) % 6                                                    # sizes: every N per region over the kinds; 'extreme' has small chroma blocks
    cls = (((k + np.where(q < 4, q, q - 3) + np.arange(n) // 6) & 3) | bits(r, 8, 3) << 2).astype(np.uint8).reshape(-1, 6)
    intra = np.where(bits(r, 12, 7) < (6 if kind == "extreme" else 3), 1 + bits(r, 16, 127) * 2, 0).astype(np.uint8).reshape(-1, 6)
    nnz = np.where(bits(r, 24, 1), 1 + bits(r, 28, 1023), 0).astype(np.uint32).reshape(-1, 6)
    span = [(20, 63), (30, 31), (0, 63), (36, 15), (0, 15), (31, 3)][k]
    qps = (span[0] + bits(r, 40, span[1])).astype(np.uint8).reshape(-1, 6)
    if kind in ("smooth", "constant"):                                      # chroma regions at the ends of the range: the tc index clamps of chroma
        qps[:, 4:] = np.where(kind == "smooth", 44 + (qps[:, 4:] & 15), qps[:, 4:] & 7)
    m = _rand(seed + 1, nb)
    base = np.stack([bits(m, 4, 15) - 8, bits(m, 8, 15) - 8], axis=1)
    mode = bits(m, 20, 15)
    mv = np.select([(mode < 8)[:, None], (mode < 11)[:, None], (mode < 14)[:, None]],
                   [np.zeros((nb, 2), np.int64) + 5, base // 4 + 5, base * 3], 0)
    ext = np.array([32767, -32768], np.int64)[bits(m, 30, 1)]
    mv = np.where((mode == 15)[:, None], np.stack([ext, -1 - ext], axis=1), mv)
    bo, to = OFFSETS[kind]
    return Side(cls, intra, nnz, qps, np.clip(mv, -32768, 32767).astype(np.int16), int(bits(r[:1], 50, 63)[0] % 52), bo, to)


# chosen on the CPU (tests/test_deblock_ref.py runs assert_coverage on the statement alone): the first value with which the kinds
# of that size together reach every counter the size allows
SEEDS = {(16, 16): 0, (32, 32): 1, (64, 64): 5, (80, 48): 1, (144, 80): 0, (272, 208): 0, (128, 64): 0}


def case(kind, w, h):
    """(y, u, v, side) of a size's case of one kind: the seeds are chosen (on the CPU, tests/test_deblock_ref.py) so that the kinds
    of a size together pass assert_coverage"""
    seed = 1000 * KINDS.index(kind) + w + 3 * h + 100000 * SEEDS[(w, h)]
    y, u, v = planes(kind, w, h, seed)
    return y, u, v, side_mix(kind, w, h, seed + 7)


def assert_coverage(w, h, counts):
    """what a size's case must have exercised, summed over its kinds.  16x16 has one crossing and no chroma edge; 32x32 has one luma
    region, so N = 32 has no transform edge there; a CTU boundary (chroma N = 32, two chroma qps at one edge) needs more than 64
    samples across the edge direction; everything else is required from 64x64 on"""
    missing = []

    def need(p, *names):
        missing.extend("%s.%s" % (p, n) for n in names if counts[p][n] <= 0)

    if (w, h) == (16, 16):
        need("luma_v", "bs0", "seg_normal")
        need("luma_h", "seg_normal")
        assert not any(counts[p]["lines"] for p in PASSES[2:])
    else:
        for p in ("luma_v", "luma_h"):
            need(p, "edges_n4", "edges_n8", "edges_n16", "edges_n32", "transform_n4", "transform_n8", "transform_n16", "not_transform")
        for p in PASSES[2:]:
            need(p, "filtered", "lines")
    if w >= 64 and h >= 48:
        for p in ("luma_v", "luma_h"):
            need(p, "bs0", "bs1", "bs2", "rule_intra", "rule_coded", "rule_motion", "seg_off", "seg_strong", "seg_normal",
                 "normal_ep0_eq0", "normal_ep0_eq1", "normal_ep1_eq0", "normal_ep1_eq1", "line_skip", "clamp_tc", "clamp_2tc", "clip8",
                 "transform_n32", "qp_differs", "beta_index_below_0", "beta_index_above_51", "tc_index_below_0", "tc_index_above_53")
        for p in PASSES[2:]:
            need(p, "not_transform", "not_intra", "clamp_tc", "clip8", "transform_n4", "transform_n8", "transform_n16", "tc_index_below_0",
                 "tc_index_above_53")
            if (w if p.endswith("_v") else h) > 64:
                need(p, "transform_n32", "qp_differs")
    assert not missing, missing
