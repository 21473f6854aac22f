"""The reference statement of mixed inter / intra coding of a frame (include/x266hip.h: xDct32CodeMixedFrameGpu), composed from the
intra frame's statement (tests/_intra_frame_ref.py: gather, the availability rules, _code_block, case), the quantiser of
tests/_quant_ref.py and the oracle's satd8x8 / intra32_costs / intra32_predict / dct32.  Nothing here is derived from the library
under test.

Inputs of the tests: cur = R.case("oriented", w, h); the prediction is cur plus +-6 noise, and in the luma regions with
(bx + by + flip) odd and in the chroma of the CTUs with (cx + cy + flip) odd it is 255 - cur: motion compensation that failed there."""
import numpy as np

import _intra_frame_ref as R
import _quant_ref as Q

NO_COST = 0xFFFFFFFF
INTER_MODE = 255


def pred_planes(w, h, flip, kind="oriented", seed=5):
    """(cur planes, pred planes) of the test frames"""
    cur = R.case(kind, w, h, seed)
    pred = []
    for i, p in enumerate(cur):
        noisy = np.clip(p.astype(np.int64) + R._noise(seed + 40 + i, p.shape, -6, 6), 0, 255).astype(np.uint8)
        edge = 32                                                           # luma: per 32x32 block; chroma: per CTU = 32 chroma samples
        by, bx = np.mgrid[0:p.shape[0], 0:p.shape[1]] // edge
        pred.append(np.where((bx + by + flip) & 1, 255 - p, noisy).astype(np.uint8))
    return cur, tuple(pred)


def kinds_mixed(n_ctu, seed=9):
    """a seeded mix of 0 / 1 / 2 with bytes above 2 (read as 2) among them"""
    r = R._noise(seed, (n_ctu, 6), 0, 7)
    return np.array([0, 1, 2, 0, 1, 2, 3, 255], np.uint8)[r]


def satd_sum(oracle, a, b):
    """the sum over the sixteen 8x8 sub-blocks of satd8x8(a - b) of two 32x32 blocks"""
    d = a.astype(np.int16) - b.astype(np.int16)
    return int(oracle.satd8x8(d.reshape(4, 8, 4, 8).transpose(0, 2, 1, 3).reshape(16, 64)).astype(np.int64).sum())


def is_intra(k, inter_cost, intra_cost, penalty):
    """step 4 of the contract: a given kind stands; a deciding region is intra iff intra_cost + penalty < inter_cost (a tie is inter)"""
    return bool(k) if k < 2 else intra_cost + penalty < inter_cost


def chroma_candidates(q0_intra, q0_mode):
    return list(R.CHROMA_CANDIDATES) + ([int(q0_mode)] if q0_intra else [])


class Mixed:
    """levels [n, 6, 1024] int16, nnz [n, 6] uint32, kinds, modes [n, 6] uint8, costs [n, 6, 2] uint32 (inter, intra), planes (y, u, v)
    of the reconstruction, candidates [n]: the chroma candidate list used (None where none was)"""

    def recon_tiles(self, oracle, base):
        out = np.array(base, np.uint8).reshape(-1, 512)
        out[:, :384] = oracle.conv_input_fmt(*self.planes).reshape(-1, 512)[:, :384]
        return out.ravel()


def _code_inter(oracle, src, pred, qp, rounding):
    coef = oracle.dct32_fwd((src.astype(np.int16) - pred.astype(np.int16)).reshape(1, 1024))
    level = Q.quant(coef, 5, qp, rounding)
    res = oracle.dct32_inv(Q.dequant(level, 5, qp).astype(np.int16)).reshape(32, 32)
    return level.astype(np.int16).ravel(), np.clip(pred.astype(np.int32) + res, 0, 255).astype(np.uint8)


def code_frame(oracle, cur, pred, w, h, qps=None, qp=0, rounding=0, penalty=0, kinds_in=None, modes_in=None):
    y, u, v = cur
    py, pu, pv = pred
    nx, ny = w // 64, h // 64
    n = nx * ny
    rq = Q.region_qp(qps, qp, 6 * n).reshape(n, 6)
    ki = np.full((n, 6), 2, np.int64) if kinds_in is None else np.minimum(np.asarray(kinds_in, np.uint8).reshape(n, 6).astype(np.int64), 2)
    mi = None if modes_in is None else np.asarray(modes_in, np.uint8).reshape(n, 6)
    ry, ru, rv = np.zeros_like(y), np.zeros_like(u), np.zeros_like(v)
    out = Mixed()
    out.levels, out.nnz = np.zeros((n, 6, 1024), np.int16), np.zeros((n, 6), np.uint32)
    out.kinds, out.modes = np.zeros((n, 6), np.uint8), np.zeros((n, 6), np.uint8)
    out.costs, out.candidates = np.full((n, 6, 2), NO_COST, np.uint32), [None] * n
    for cy in range(ny):
        for cx in range(nx):
            ctu = cy * nx + cx
            for q in range(4):
                bx, by = 2 * cx + (q & 1), 2 * cy + (q >> 1)
                k = int(ki[ctu, q])
                win = (slice(32 * by, 32 * by + 32), slice(32 * bx, 32 * bx + 32))
                src, prd = y[win], py[win]
                inter_cost = intra_cost = NO_COST
                mode = INTER_MODE
                if k >= 1:
                    refs = R.gather(ry, 32 * bx, 32 * by, R.luma_availability(bx, by, 2 * nx, 2 * ny))
                    if mi is None:
                        costs, best = oracle.intra32_costs(refs[None], src.reshape(1, 1024))
                        mode, intra_cost = int(best[0]), int(costs[0][best[0]])
                        assert intra_cost == int(costs[0].min()) and mode == int(np.argmin(costs[0]))   # the lowest index wins ties
                    else:
                        mode = int(mi[ctu, q])
                        if k == 2:
                            intra_cost = int(oracle.intra32_costs(refs[None], src.reshape(1, 1024))[0][0][mode])
                if k == 2:
                    inter_cost = satd_sum(oracle, src, prd)
                intra = is_intra(k, inter_cost, intra_cost, penalty)
                if intra:
                    _, level, rec = R._code_block(oracle, refs, src, mode, int(rq[ctu, q]), rounding)
                else:
                    level, rec = _code_inter(oracle, src, prd, int(rq[ctu, q]), rounding)
                ry[win] = rec
                out.levels[ctu, q], out.nnz[ctu, q] = level, np.count_nonzero(level)
                out.kinds[ctu, q], out.modes[ctu, q] = intra, mode if intra else INTER_MODE
                out.costs[ctu, q] = (inter_cost, intra_cost)
            k = int(ki[ctu, 4])
            win = (slice(32 * cy, 32 * cy + 32), slice(32 * cx, 32 * cx + 32))
            srcs, prds = [p[win] for p in (u, v)], [p[win] for p in (pu, pv)]
            inter_cost = intra_cost = NO_COST
            mode = INTER_MODE
            if k >= 1:
                avail = R.chroma_availability(cx, cy, nx)
                sets = [R.gather(p, 32 * cx, 32 * cy, avail) for p in (ru, rv)]
                if mi is None or k == 2:
                    costs = [oracle.intra32_costs(sets[i][None], srcs[i].reshape(1, 1024))[0][0].astype(np.int64) for i in range(2)]
                if mi is None:
                    cand = chroma_candidates(out.kinds[ctu, 0], out.modes[ctu, 0])
                    out.candidates[ctu] = cand
                    total = [int(costs[0][m] + costs[1][m]) for m in cand]
                    intra_cost = min(total)
                    mode = cand[total.index(intra_cost)]                    # the first in the list wins ties
                else:
                    mode = int(mi[ctu, 4])
                    if k == 2:
                        intra_cost = int(costs[0][mode] + costs[1][mode])
            if k == 2:
                inter_cost = satd_sum(oracle, srcs[0], prds[0]) + satd_sum(oracle, srcs[1], prds[1])
            intra = is_intra(k, inter_cost, intra_cost, penalty)
            for i, rp in enumerate((ru, rv)):
                if intra:
                    _, level, rec = R._code_block(oracle, sets[i], srcs[i], mode, int(rq[ctu, 4 + i]), rounding)
                else:
                    level, rec = _code_inter(oracle, srcs[i], prds[i], int(rq[ctu, 4 + i]), rounding)
                rp[win] = rec
                out.levels[ctu, 4 + i], out.nnz[ctu, 4 + i] = level, np.count_nonzero(level)
                out.kinds[ctu, 4 + i], out.modes[ctu, 4 + i] = intra, mode if intra else INTER_MODE
                out.costs[ctu, 4 + i] = (inter_cost, intra_cost)
    out.planes = (ry, ru, rv)
    return out


_cache = {}


def coded(oracle, w, h, flip, penalty=0, kinds=None, qp=22, rounding=171):
    """code_frame of the test frames at a scalar qp with the call choosing the modes, computed once and shared between the tests; kinds is
    None, an int (every region) or "mixed"; do not modify the result"""
    key = (w, h, flip, penalty, kinds, qp, rounding)
    if key not in _cache:
        cur, pred = pred_planes(w, h, flip)
        n = (w // 64) * (h // 64)
        ki = None if kinds is None else kinds_mixed(n) if kinds == "mixed" else np.full((n, 6), kinds, np.uint8)
        _cache[key] = code_frame(oracle, cur, pred, w, h, None, qp, rounding, penalty, ki)
    return _cache[key]
