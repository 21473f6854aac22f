"""A decoder of a coded frame in numpy, from what a decoder would have and nothing else: the packed level records and stream
(xLevelsPackGpu), the kinds and modes of the regions, the qp bytes (or the scalar qp), and the prediction planes for the inter regions.
Built from the statements the coding calls are tested against -- tests/_levels_ref.py's unpack, tests/_quant_ref.py's dequant, the
oracle's inverse DCT32 and intra predictor, tests/_intra_frame_ref.py's gather -- in the order the header gives for a CTU: the four luma
regions in Z order, then U, then V, every intra region predicted from the frame as rebuilt so far."""
import numpy as np

import _intra_frame_ref as R
import _levels_ref as V
import _quant_ref as Q


def _rebuild(oracle, pred, level, qp):
    res = oracle.dct32_inv(Q.dequant(level.astype(np.int64), 5, qp).astype(np.int16).reshape(1, 1024)).reshape(32, 32)
    return np.clip(pred.astype(np.int32) + res, 0, 255).astype(np.uint8)


def _intra(oracle, plane, x0, y0, avail, mode):
    refs = R.gather(plane, x0, y0, avail)
    return oracle.intra32_predict(refs[None, :129], np.array([mode], np.uint8)).reshape(32, 32)


def decode(oracle, records, stream, w, h, kinds, modes, qps=None, qp=0, pred_planes=None):
    """-> ((y, u, v) of the rebuilt frame, levels [n_ctu, 6, 1024] int16 as unpacked).  kinds, modes: [n_ctu, 6] (a kind other than 0 is
    intra; entry 5 of either is not looked at: V follows U); pred_planes may be None when no region is inter"""
    nx, ny = w // 64, h // 64
    n = nx * ny
    levels = V.unpack(records, stream, 6 * n)[0].reshape(n, 6, 1024)
    kinds, modes = np.asarray(kinds, np.uint8).reshape(n, 6), np.asarray(modes, np.uint8).reshape(n, 6)
    rq = Q.region_qp(qps, qp, 6 * n).reshape(n, 6)
    y, u, v = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)
    for cy in range(ny):
        for cx in range(nx):
            ctu = cy * nx + cx
            for q in range(4):
                bx, by = 2 * cx + (q & 1), 2 * cy + (q >> 1)
                win = (slice(32 * by, 32 * by + 32), slice(32 * bx, 32 * bx + 32))
                if kinds[ctu, q]:
                    pred = _intra(oracle, y, 32 * bx, 32 * by, R.luma_availability(bx, by, 2 * nx, 2 * ny), int(modes[ctu, q]))
                else:
                    pred = pred_planes[0][win]
                y[win] = _rebuild(oracle, pred, levels[ctu, q], int(rq[ctu, q]))
            win = (slice(32 * cy, 32 * cy + 32), slice(32 * cx, 32 * cx + 32))
            for i, plane in enumerate((u, v)):
                if kinds[ctu, 4]:
                    pred = _intra(oracle, plane, 32 * cx, 32 * cy, R.chroma_availability(cx, cy, nx), int(modes[ctu, 4]))
                else:
                    pred = pred_planes[1 + i][win]
                plane[win] = _rebuild(oracle, pred, levels[ctu, 4 + i], int(rq[ctu, 4 + i]))
    return (y, u, v), levels
