"""The reference statement of intra coding on tiled frames (include/x266hip.h: xIntra32RefsFromTilesGpu, xIntra32CodeFrameGpu),
composed from the oracle's intra32_costs / intra32_predict / dct32_fwd / dct32_inv / conv_input_fmt / conv_output_420 and the
quantiser of tests/_quant_ref.py; the gather rule is plain per-sample code.  Nothing here is derived from the library under test.

SIZES are the smallest frames that contain a block with no neighbour at all, every frame-edge case, a quadrant 1 whose TR comes
from CTU (cx+1, cy-1) and one whose TR is outside the frame, and a quadrant 0 with BL from the left CTU."""
import numpy as np

import _quant_ref as Q
from _util import splitmix64

SIZES = ((64, 64), (128, 64), (64, 128), (128, 128), (192, 128))
KINDS = ("oriented", "noise", "flat", "extreme")
CHROMA_CANDIDATES = (0, 26, 10, 1)                                          # and, fifth, the mode chosen for quadrant 0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _noise(seed, shape, lo, hi):
    r = (splitmix64(seed, 0, shape[0] * shape[1]) >> np.uint64(13)).astype(np.int64).reshape(shape)
    return lo + r % (hi - lo + 1)


def case(kind, w, h, seed=5):
    """(y, u, v) planes of a w x h 4:2:0 frame"""
    if kind == "flat":
        return np.full((h, w), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)
    if kind == "noise":
        return (_noise(seed + 10, (h, w), 0, 255).astype(np.uint8), _noise(seed + 11, (h // 2, w // 2), 0, 255).astype(np.uint8),
                _noise(seed + 12, (h // 2, w // 2), 0, 255).astype(np.uint8))
    if kind == "extreme":                                                   # 8x8 patches of 0 / 255: every clip of the loop
        def patches(s, hh, ww):
            return (np.kron(_noise(s, (hh // 8, ww // 8), 0, 1), np.ones((8, 8), np.int64)) * 255).astype(np.uint8)
        y = patches(seed + 20, h, w)
        y[:32, :32] = 128                                                   # the block without neighbours codes nothing, next to blocks that do
        return y, patches(seed + 21, h // 2, w // 2), patches(seed + 22, h // 2, w // 2)
    assert kind == "oriented"
    # per 32x32 block a sinusoid at a block-dependent angle plus +-4 noise; in CTUs with cx + cy odd one angle for the whole CTU.
    # U = the 2:1 mean of luma, V its complement: the luma mode of quadrant 0 (DM) can win the chroma decision
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w), float)
    for by in range(h // 32):
        for bx in range(w // 32):
            cx, cy = bx // 2, by // 2
            whole = (cx + cy) & 1
            k = (cy * (w // 64) + cx) * 5 + 3 if whole else by * (w // 32) + bx
            ang = np.pi * ((k * 7) % 16) / 16.0
            ys, xs = yy[by * 32:by * 32 + 32, bx * 32:bx * 32 + 32], xx[by * 32:by * 32 + 32, bx * 32:bx * 32 + 32]
            img[by * 32:by * 32 + 32, bx * 32:bx * 32 + 32] = 128 + 90 * np.sin((xs * np.cos(ang) + ys * np.sin(ang)) * 0.35 + (0 if whole else k))
    sub = img.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    y = np.clip(img + _noise(seed, img.shape, -4, 4), 0, 255).astype(np.uint8)
    u = np.clip(sub + _noise(seed + 1, sub.shape, -4, 4), 0, 255).astype(np.uint8)
    v = np.clip(255 - sub + _noise(seed + 2, sub.shape, -4, 4), 0, 255).astype(np.uint8)
    return y, u, v


def tiles(oracle, planes, seed):
    """the tile array of three planes with random m_I bytes (which no call may read)"""
    t = oracle.conv_input_fmt(*planes).reshape(-1, 512)
    t[:, 384:] = (splitmix64(seed, 0, t.shape[0] * 128) & np.uint64(255)).astype(np.uint8).reshape(-1, 128)
    return t.ravel()


def planes_of_tiles(oracle, t, w, h):
    return oracle.conv_output_420(t, w, h)


# ---- the gather rule -------------------------------------------------------------------------------------------------------------------
def luma_availability(bx, by, blocks_x, blocks_y):
    """(BL, L, C, T, TR) of luma block (bx, by) on the 32-sample grid"""
    q = 2 * (by & 1) + (bx & 1)
    inside = lambda x, y: 0 <= x < blocks_x and 0 <= y < blocks_y
    return (inside(bx - 1, by + 1) and q == 0, inside(bx - 1, by), inside(bx - 1, by - 1), inside(bx, by - 1), inside(bx + 1, by - 1) and q != 3)


def chroma_availability(cx, cy, ctus_x):
    return (False, cx > 0, cx > 0 and cy > 0, cy > 0, cy > 0 and cx + 1 < ctus_x)


def gather(plane, x0, y0, avail):
    """the 129 samples left[64] | top[65] of the 32x32 block at (x0, y0) of `plane`, segments available as in `avail`"""
    bl, l, c, t, tr = avail
    seq, ok = [], []
    for i in range(129):                                                    # the scan: left[63] .. left[0], top[0] .. top[64]
        if i < 64:
            x, y, a = x0 - 1, y0 + 63 - i, (bl if 63 - i >= 32 else l)
        elif i == 64:
            x, y, a = x0 - 1, y0 - 1, c
        else:
            x, y, a = x0 + i - 65, y0 - 1, (t if i - 65 < 32 else tr)
        ok.append(bool(a))
        seq.append(int(plane[y, x]) if a else -1)
    if not any(ok):
        seq = [128] * 129
    else:
        first = ok.index(True)
        for i in range(first):
            seq[i] = seq[first]
        for i in range(first + 1, 129):
            if not ok[i]:
                seq[i] = seq[i - 1]
    return np.array(seq[63::-1] + seq[64:], np.uint8)


def _sets(rows):
    out = np.zeros((len(rows), 144), np.uint8)                              # the 15 reserved bytes are written as 0
    out[:, :129] = np.array(rows, np.uint8).reshape(len(rows), 129)
    return out


def refs_from_planes(planes, w, h, component):
    """what xIntra32RefsFromTilesGpu writes: uint8 [n_sets, 144]"""
    nx, ny = w // 64, h // 64
    rows = []
    for cy in range(ny):
        for cx in range(nx):
            if component == 0:
                for q in range(4):
                    bx, by = 2 * cx + (q & 1), 2 * cy + (q >> 1)
                    rows.append(gather(planes[0], 32 * bx, 32 * by, luma_availability(bx, by, 2 * nx, 2 * ny)))
            else:
                rows.append(gather(planes[component], 32 * cx, 32 * cy, chroma_availability(cx, cy, nx)))
    return _sets(rows)


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------
class Coded:
    """levels [n, 6, 1024] int16, nnz [n, 6] uint32, modes [n, 6] uint8, planes (y, u, v) of the reconstruction, chroma_pos [n]: the
    winning position in the chroma candidate list (-1 with modes given), preds [n, 6, 1024] uint8 and refs [n, 6, 129] as used"""

    def recon_tiles(self, oracle, base):
        out = np.array(base, np.uint8).reshape(-1, 512)
        out[:, :384] = oracle.conv_input_fmt(*self.planes).reshape(-1, 512)[:, :384]
        return out.ravel()


def _code_block(oracle, refs, src, mode, qp, rounding):
    pred = oracle.intra32_predict(refs[None, :129], np.array([mode], np.uint8)).reshape(32, 32)
    coef = oracle.dct32_fwd((src.astype(np.int16) - pred.astype(np.int16)).reshape(1, 1024))
    level = Q.quant(coef, 5, qp, rounding)
    res = oracle.dct32_inv(Q.dequant(level, 5, qp).astype(np.int16)).reshape(32, 32)
    return pred, level.astype(np.int16).ravel(), np.clip(pred.astype(np.int32) + res, 0, 255).astype(np.uint8)


def code_frame(oracle, planes, w, h, qps=None, qp=0, rounding=0, modes_in=None):
    y, u, v = planes
    nx, ny = w // 64, h // 64
    n = nx * ny
    rq = Q.region_qp(qps, qp, 6 * n).reshape(n, 6)
    mi = None if modes_in is None else np.asarray(modes_in, np.uint8).reshape(n, 6)
    ry, ru, rv = np.zeros_like(y), np.zeros_like(u), np.zeros_like(v)
    out = Coded()
    out.levels, out.nnz, out.modes = np.zeros((n, 6, 1024), np.int16), np.zeros((n, 6), np.uint32), np.zeros((n, 6), np.uint8)
    out.chroma_pos, out.preds, out.refs = np.full(n, -1), np.zeros((n, 6, 1024), np.uint8), np.zeros((n, 6, 129), np.uint8)
    for cy in range(ny):
        for cx in range(nx):
            ctu = cy * nx + cx
            for q in range(4):
                bx, by = 2 * cx + (q & 1), 2 * cy + (q >> 1)
                refs = gather(ry, 32 * bx, 32 * by, luma_availability(bx, by, 2 * nx, 2 * ny))
                src = y[32 * by:32 * by + 32, 32 * bx:32 * bx + 32]
                mode = int(oracle.intra32_costs(refs[None], src.reshape(1, 1024))[1][0]) if mi is None else int(mi[ctu, q])
                pred, level, rec = _code_block(oracle, refs, src, mode, int(rq[ctu, q]), rounding)
                ry[32 * by:32 * by + 32, 32 * bx:32 * bx + 32] = rec
                out.levels[ctu, q], out.nnz[ctu, q], out.modes[ctu, q] = level, np.count_nonzero(level), mode
                out.preds[ctu, q], out.refs[ctu, q] = pred.ravel(), refs
            avail = chroma_availability(cx, cy, nx)
            sets = [gather(p, 32 * cx, 32 * cy, avail) for p in (ru, rv)]
            srcs = [p[32 * cy:32 * cy + 32, 32 * cx:32 * cx + 32] for p in (u, v)]
            if mi is None:
                cand = list(CHROMA_CANDIDATES) + [int(out.modes[ctu, 0])]
                costs = [oracle.intra32_costs(sets[k][None], srcs[k].reshape(1, 1024))[0][0].astype(np.int64) for k in range(2)]
                total = [int(costs[0][m] + costs[1][m]) for m in cand]
                pos = total.index(min(total))                               # the first in the list wins ties
                mode, out.chroma_pos[ctu] = cand[pos], pos
            else:
                mode = int(mi[ctu, 4])
            for k, rp in enumerate((ru, rv)):
                pred, level, rec = _code_block(oracle, sets[k], srcs[k], mode, int(rq[ctu, 4 + k]), rounding)
                rp[32 * cy:32 * cy + 32, 32 * cx:32 * cx + 32] = rec
                out.levels[ctu, 4 + k], out.nnz[ctu, 4 + k], out.modes[ctu, 4 + k] = level, np.count_nonzero(level), mode
                out.preds[ctu, 4 + k], out.refs[ctu, 4 + k] = pred.ravel(), sets[k]
    out.planes = (ry, ru, rv)
    return out


_cache = {}


def coded(oracle, kind, w, h, qp=22, rounding=171):
    """code_frame of case(kind, w, h) at a scalar qp, computed once and shared between the tests; do not modify the result"""
    key = (kind, w, h, qp, rounding)
    if key not in _cache:
        _cache[key] = code_frame(oracle, case(kind, w, h), w, h, None, qp, rounding)
    return _cache[key]
