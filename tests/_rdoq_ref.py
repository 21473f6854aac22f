"""Rate-distortion optimised quantisation and the level rate estimate of include/x266hip.h (xRdoQuantRegionsGpu, xLevelsBitsGpu,
xLevelBits, xLastPosBits, xCgFlagBits) in plain numpy int64, written from the header's text: the tables, R, Rlast, D, J, steps 1 to 3
block by block with every sum of the statement taken as the sum it names (step 3's Totals as differences of running sums).  Nothing
here is derived from the library under test; f and qbits come from _quant_ref, the scan from _levels_ref."""
import functools

import numpy as np

import _levels_ref as lref
import _quant_ref as qref

SIG = ((24, 10), (12, 22), (6, 36))
GT1 = (10, 24)
GT2 = (11, 22)
CGF = (9, 26)
SIGN = 16
LAMBDA_MAX = 8192
STAT_DTYPE = np.dtype([("dist", "<u8"), ("bits", "<u4"), ("n_nz", "<u4")])
assert STAT_DTYPE.itemsize == 16


def ilog2(t):
    assert t >= 1
    return int(t).bit_length() - 1


def rem_bits(r):
    return r + 1 if r < 3 else 3 + 2 * ilog2(r - 2) + 1


def level_bits(l, cls):
    """R(l, class) in 1/16 bit"""
    if l == 0:
        return SIG[cls][0]
    if l == 1:
        return SIG[cls][1] + SIGN + GT1[0]
    if l == 2:
        return SIG[cls][1] + SIGN + GT1[1] + GT2[0]
    return SIG[cls][1] + SIGN + GT1[1] + GT2[1] + 16 * rem_bits(l - 3)


def pos_bits(t, n):
    g = t if t < 4 else 2 * ilog2(t) + ((t >> (ilog2(t) - 1)) & 1)
    return min(g + 1, 2 * n - 1) + ((g >> 1) - 1 if g >= 4 else 0)


def last_pos_bits(u, v, n):
    """Rlast(u, v) of a block of 1 << n"""
    return 16 * (pos_bits(u, n) + pos_bits(v, n))


def cg_flag_bits(coded):
    return CGF[coded]


@functools.lru_cache(None)
def _rate_table():
    """[3, 32769]: R(l, class) for every magnitude an int16 level has"""
    return np.array([[level_bits(l, c) for l in range(32769)] for c in range(3)], np.int64)


@functools.lru_cache(None)
def _block_geometry(n):
    """per scan index i of a block of N = 1 << n: its offset v * N + u inside the block, position class, Rlast"""
    size = 1 << n
    off = lref.scan(size)
    u, v = off % size, off // size
    cls = np.where((u == 0) & (v == 0), 0, np.where((u < 4) & (v < 4), 1, 2))
    rlast = np.array([last_pos_bits(int(a), int(b), n) for a, b in zip(u, v)], np.int64)
    return off, cls, rlast


def dist(x, l, qb):
    """D(l) for x = |c| * f: numpy int64"""
    err = np.abs(x - (np.asarray(l, np.int64) << qb))
    e = (err + (np.int64(1) << (qb - 9))) >> (qb - 8)
    return e * e


def block_bits(mag, n):
    """`bits` of one block from its level magnitudes in scan order alone; 0 for an all-zero block"""
    _, cls, rlast = _block_geometry(n)
    rate = _rate_table()
    nz = np.flatnonzero(mag)
    if nz.size == 0:
        return 0
    p = int(nz[-1])
    sp = p // 16
    bits = int(rlast[p]) - SIG[cls[p]][1]
    for s in range(sp + 1):
        lo, hi = 16 * s, min(16 * s + 15, p)
        coded = bool(mag[16 * s:16 * s + 16].any())
        if 0 < s < sp:
            bits += CGF[coded]
        if s == 0 or s == sp or coded:
            bits += int(rate[cls[lo:hi + 1], mag[lo:hi + 1]].sum())
    return bits


def rdoq_block(c, n, qp, lam, steps=3, totals=None, cgs=None):
    """one block's coefficients in scan order -> (levels in scan order, dist, bits, changed from h, CGs zeroed, last moved or gone).
    steps < 3 stops after that step (the hand-worked cases look at one rule at a time); totals: a dict that receives Total(p) of
    step 3, Total(none) under the key None; cgs: a dict that receives (Jz, Jc) of every CG that step 2 weighs."""
    _, cls, rlast = _block_geometry(n)
    rate = _rate_table()
    c = np.asarray(c, np.int64)
    qb = int(qref.qbits(n, qp))
    x = np.abs(c) * int(qref.F[qp % 6])
    lam = int(lam)
    # step 1
    h = (x + (np.int64(1) << (qb - 1))) >> qb
    q = h.copy()
    best = dist(x, h, qb) + lam * rate[cls, h]
    for cand, allowed in ((np.maximum(h - 1, 0), h >= 1), (np.zeros_like(h), h <= 2)):   # descending levels: "<=" lets the smaller one win a tie
        j = dist(x, cand, qb) + lam * rate[cls, cand]
        take = allowed & (cand < q) & (j <= best)
        q = np.where(take, cand, q)
        best = np.where(take, j, best)
    changed = int(np.count_nonzero(q != h))
    d0 = dist(x, 0, qb)
    jq = lambda: dist(x, q, qb) + lam * rate[cls, q]
    n_cg = c.size // 16
    # step 2
    zeroed = 0
    j1 = jq()                                                                   # a CG is weighed before any of its levels goes
    for s in range(1, n_cg if steps >= 2 else 0):
        sl = slice(16 * s, 16 * s + 16)
        if not q[sl].any():
            continue
        jc = int(j1[sl].sum()) + lam * CGF[1]
        jz = int(d0[sl].sum()) + lam * CGF[0]
        if cgs is not None:
            cgs[s] = (jz, jc)
        if jz < jc:
            q[sl] = 0
            zeroed += 1
    # step 3
    moved = 0
    if steps >= 3 and q.any():
        j = jq()
        dq = dist(x, q, qb)
        cost = []
        for s in range(n_cg):
            sl = slice(16 * s, 16 * s + 16)
            if s == 0:
                cost.append(int(j[sl].sum()))
            elif q[sl].any():
                cost.append(int(j[sl].sum()) + lam * CGF[1])
            else:
                cost.append(int(d0[sl].sum()) + lam * CGF[0])
        # Total(p) = the CGs before p's + J of p's CG before p + D(q[p]) + lambda (R - sig1) + D(0) behind p + lambda Rlast(p), each sum
        # as a difference of two running sums (int64 holds them: a block's D(0) stays below 2^55)
        nz = np.flatnonzero(q)
        sp = nz // 16
        cg_before = np.concatenate(([0], np.cumsum(np.array(cost, np.int64))))
        j_before = np.concatenate(([0], np.cumsum(j)))
        d0_behind = int(d0.sum()) - np.cumsum(d0)
        sig1 = np.array([sig[1] for sig in SIG], np.int64)
        total_of = cg_before[sp] + j_before[nz] - j_before[16 * sp] + dq[nz] + lam * (rate[cls[nz], q[nz]] - sig1[cls[nz]]) + d0_behind[nz] + lam * rlast[nz]
        best_p, best_total = None, int(d0.sum())                                # Total(none)
        for p, total in zip(nz.tolist(), total_of.tolist()):
            if totals is not None:
                totals[p], totals[None] = total, int(d0.sum())
            if total <= best_total:                                            # ascending p: the larger wins a tie, any p wins over none
                best_p, best_total = p, total
        if best_p is None:
            q[:] = 0
            moved = 1
        else:
            moved = int(best_p != int(np.flatnonzero(q)[-1]))
            q[best_p + 1:] = 0
    return np.sign(c) * q, int(dist(x, q, qb).sum()), block_bits(q, n), changed, zeroed, moved


def step3_choice(totals, bits=64):
    """the position step 3 keeps as the last one (None: no level stays), from the Totals that rdoq_block hands out, each taken modulo
    2^bits: 64 is the statement, 32 what a comparison of the low dwords alone would choose"""
    mask = (1 << bits) - 1
    best_p, best_total = None, totals[None] & mask
    for p in sorted(k for k in totals if k is not None):
        if totals[p] & mask <= best_total:
            best_p, best_total = p, totals[p] & mask
    return best_p


def _region_blocks(k):
    """[(32 / N)^2, N * N]: the index inside a region of class k of scan position i of block b"""
    size = 4 << k
    return lref.region_order(k).reshape(-1, size * size)


def rdo_quant(coef, classes=None, qps=None, qp=0, lam=368):
    """-> (levels int16 [n, 1024], stats STAT_DTYPE [n], counters): counters = {"changed", "cg_zeroed", "last_moved"} summed over the batch"""
    x = np.asarray(coef, np.int16).reshape(-1, 1024).astype(np.int64)
    nr = x.shape[0]
    n_of = qref.region_n(classes, nr)
    qp_of = qref.region_qp(qps, qp, nr)
    out = np.zeros((nr, 1024), np.int64)
    stat = np.zeros(nr, STAT_DTYPE)
    counters = {"changed": 0, "cg_zeroed": 0, "last_moved": 0}
    for r in range(nr):
        n = int(n_of[r])
        d_sum = b_sum = 0
        for idx in _region_blocks(n - 2):
            lv, d, b, changed, zeroed, moved = rdoq_block(x[r, idx], n, int(qp_of[r]), lam)
            out[r, idx] = lv
            d_sum += d
            b_sum += b
            counters["changed"] += changed
            counters["cg_zeroed"] += zeroed
            counters["last_moved"] += moved
        stat[r] = (d_sum, b_sum, np.count_nonzero(out[r]))
    return out.astype(np.int16), stat, counters


def levels_bits(levels, classes=None, nnz=None):
    """xLevelsBitsGpu -> stats STAT_DTYPE [n] (dist 0); a region with nnz[r] == 0 reports zeros"""
    lv = np.abs(np.asarray(levels, np.int16).reshape(-1, 1024).astype(np.int64))
    nr = lv.shape[0]
    n_of = qref.region_n(classes, nr)
    stat = np.zeros(nr, STAT_DTYPE)
    for r in range(nr):
        if nnz is not None and int(np.asarray(nnz).ravel()[r]) == 0:
            continue
        n = int(n_of[r])
        stat[r] = (0, sum(block_bits(lv[r, idx], n) for idx in _region_blocks(n - 2)), np.count_nonzero(lv[r]))
    return stat


# ---- the fixtures the CPU and the GPU tests share ---------------------------------------------------------------------------------------
def laplacian(n_regions, classes=None, qps=None, qp=0, dc_levels=16.0, seed=1):
    """[n_regions, 1024] int16: Laplacian coefficients whose scale decays as 1 / (1 + (u + v) / 2) from `dc_levels` quantiser steps of
    the region's own block size and qp at DC, clipped to int16"""
    rng = np.random.RandomState(seed)
    n_of = qref.region_n(classes, n_regions)
    qp_of = qref.region_qp(qps, qp, n_regions)
    out = np.zeros((n_regions, 1024), np.float64)
    for r in range(n_regions):
        n, q = int(n_of[r]), int(qp_of[r])
        size = 1 << n
        step = float(1 << int(qref.qbits(n, q))) / float(qref.F[q % 6])
        v, u = np.divmod(np.arange(size * size), size)
        decay = np.tile(dc_levels * step / (1.0 + (u + v) / 2.0), 1024 // (size * size))
        out[r] = np.rint(rng.laplace(0.0, 1.0, 1024) * decay)
    return np.clip(out, -32768, 32767).astype(np.int16)


def edge_regions(k):
    """five regions of class k: all zero, every coefficient -32768, every coefficient +32767, a single non-zero at u = v = N - 1 of
    block 0, a single non-zero at DC of block 0"""
    size = 4 << k
    x = np.zeros((5, 1024), np.int16)
    x[1] = -32768
    x[2] = 32767
    x[3, size * size - 1] = 3000
    x[4, 0] = -3000
    return x
