"""The reference statement of the quantiser (include/x266hip.h, xQuantRegionsGpu) in numpy int64, and of the fused CTU coding call
composed from it with the oracle's dct32 / dct32_inv / conv_input_fmt.  For an N x N block, n = log2 N in 2..5, qp in 0..51,
rounding in 0..511:

    qbits = 14 + qp/6 + (7 - n)
    level = sign(c) * ((|c| * F[qp%6] + (rounding << (qbits - 9))) >> qbits)
    coef' = clip_int16((level * (G[qp%6] << (qp/6)) + (1 << (n - 2))) >> (n - 1))

Nothing here is derived from the library under test."""
import numpy as np

from _util import splitmix64

F = np.array([26214, 23302, 20560, 18396, 16384, 14564], np.int64)
G = np.array([40, 45, 51, 57, 64, 72], np.int64)


def qbits(n, qp):
    return 14 + np.asarray(qp, np.int64) // 6 + (7 - np.asarray(n, np.int64))


def quant_unsigned(mag, n, qp, rounding):
    """(|c| * f + offset) >> qbits and the value before the shift, int64 (n, qp broadcast against mag)"""
    qp = np.asarray(qp, np.int64)
    qb = qbits(n, qp)
    pre = np.asarray(mag, np.int64) * F[qp % 6] + (np.int64(rounding) << (qb - 9))
    return pre >> qb, pre


def quant(c, n, qp, rounding):
    c = np.asarray(c, np.int64)
    return np.sign(c) * quant_unsigned(np.abs(c), n, qp, rounding)[0]


def dequant_unclipped(level, n, qp):
    qp, n = np.asarray(qp, np.int64), np.asarray(n, np.int64)
    scale = G[qp % 6] << (qp // 6)
    prod = np.asarray(level, np.int64) * scale
    return (prod + (np.int64(1) << (n - 2))) >> (n - 1), prod          # numpy's >> on int64 is arithmetic


def dequant(level, n, qp):
    return np.clip(dequant_unclipped(level, n, qp)[0], -32768, 32767)


def region_n(classes, n_regions):
    """log2 N per region: the low two bits of the class byte + 2 (X266_TILE_CLASS), 5 without class bytes"""
    if classes is None:
        return np.full(n_regions, 5, np.int64)
    return 2 + (np.asarray(classes, np.uint8).ravel().astype(np.int64) & 3)


def region_qp(qps, qp, n_regions):
    if qps is None:
        return np.full(n_regions, qp, np.int64)
    return np.minimum(np.asarray(qps, np.uint8).ravel().astype(np.int64), 51)


def quant_regions(x, inverse=False, classes=None, qps=None, qp=0, rounding=0):
    """[n_regions, 1024] int16 -> (levels int16, nnz uint32) forward, coefficients int16 inverse"""
    x = np.asarray(x, np.int16).reshape(-1, 1024)
    n = region_n(classes, x.shape[0])[:, None]
    q = region_qp(qps, qp, x.shape[0])[:, None]
    if inverse:
        return dequant(x, n, q).astype(np.int16)
    lv = quant(x, n, q, rounding)
    assert np.abs(lv).max(initial=0) <= 13108
    return lv.astype(np.int16), np.count_nonzero(lv, axis=1).astype(np.uint32)


# ---- the fused CTU call -------------------------------------------------------------------------------------------------------------
def _planes(tiles, w, h):
    """(y, u, v) planes held by a tile array (the inverse of xConvInputFmt's packing)"""
    t = np.asarray(tiles, np.uint8).reshape(h // 16, w // 16, 512)
    y = t[:, :, :256].reshape(h // 16, w // 16, 16, 16).transpose(0, 2, 1, 3).reshape(h, w)
    c = t[:, :, 256:384].reshape(h // 16, w // 16, 8, 8, 2).transpose(0, 2, 1, 3, 4).reshape(h // 2, w // 2, 2)
    return y, c[..., 0].copy(), c[..., 1].copy()


def _clip(pred, res):
    return np.clip(pred.astype(np.int32) + res.astype(np.int32), 0, 255).astype(np.uint8)


def _regions_of_planes(y, u, v, w, h):
    """[n_ctus, 6, 32, 32]: Y0 Y1 Y2 Y3 U V of every 64x64 CTU in raster order (w, h multiples of 64)"""
    ny, nx = h // 64, w // 64
    out = np.empty((ny, nx, 6, 32, 32), y.dtype)
    out[:, :, :4] = y.reshape(ny, 2, 32, nx, 2, 32).transpose(0, 3, 1, 4, 2, 5).reshape(ny, nx, 4, 32, 32)
    out[:, :, 4] = u.reshape(ny, 32, nx, 32).transpose(0, 2, 1, 3)
    out[:, :, 5] = v.reshape(ny, 32, nx, 32).transpose(0, 2, 1, 3)
    return out.reshape(-1, 6, 32, 32)


def _planes_of_regions(reg, w, h):
    ny, nx = h // 64, w // 64
    r = np.asarray(reg).reshape(ny, nx, 6, 32, 32)
    y = r[:, :, :4].reshape(ny, nx, 2, 2, 32, 32).transpose(0, 2, 4, 1, 3, 5).reshape(h, w)
    u = r[:, :, 4].transpose(0, 2, 1, 3).reshape(h // 2, w // 2)
    v = r[:, :, 5].transpose(0, 2, 1, 3).reshape(h // 2, w // 2)
    return y, u, v


def ctu_coefficients(oracle, cur, pred, w, h):
    """[n_ctus * 6, 1024] int16: DCT32(cur - pred) of every region"""
    cy, cu, cv = _planes(cur, w, h)
    py, pu, pv = _planes(pred, w, h)
    d = lambda a, b: a.astype(np.int16) - b.astype(np.int16)
    return oracle.dct32_fwd(_regions_of_planes(d(cy, py), d(cu, pu), d(cv, pv), w, h).reshape(-1, 1024))


def recon_of_coefficients(oracle, coef, pred, base, w, h):
    """the tile array after clamp(pred + IDCT32(coef), 0, 255) went into m_Y / m_C of `base`"""
    ry, ru, rv = _planes_of_regions(oracle.dct32_inv(np.asarray(coef, np.int16).reshape(-1, 1024)), w, h)
    py, pu, pv = _planes(pred, w, h)
    packed = oracle.conv_input_fmt(_clip(py, ry), _clip(pu, ru), _clip(pv, rv)).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    out[:, :384] = packed[:, :384]
    return out.ravel()


def code_ctu_tiles(oracle, cur, pred, w, h, qps=None, qp=0, rounding=0, base=None):
    """(levels [n_ctus, 6, 1024] int16, nnz [n_ctus, 6] uint32, recon tile array) of xDct32CodeCtuTilesGpu; m_I comes from `base`
    (None: pred's)"""
    level, nnz = quant_regions(ctu_coefficients(oracle, cur, pred, w, h), False, None, qps, qp, rounding)
    coef = quant_regions(level, True, None, qps, qp)
    recon = recon_of_coefficients(oracle, coef, pred, pred if base is None else base, w, h)
    return level.reshape(-1, 6, 1024), nnz.reshape(-1, 6), recon


# ---- data recipes of the GPU tests ----------------------------------------------------------------------------------------------------
EXTREMES = np.array([32767, -32767, -32768, 255, -255, 256, -256, 0], np.int16)


def _res_mix(n, seed):
    """int16 samples: a quarter each full range, the extremes of EXTREMES, small (-256..255) and +-1 / 0"""
    r = splitmix64(seed, 0, n)
    kind = r & np.uint64(3)
    full = (r >> np.uint64(16)).astype(np.uint16).view(np.int16)
    ext = EXTREMES[((r >> np.uint64(48)) % np.uint64(len(EXTREMES))).astype(np.int64)]
    small = ((r >> np.uint64(32)) & np.uint64(0x1FF)).astype(np.int16) - np.int16(256)
    tiny = ((r >> np.uint64(40)) % np.uint64(3)).astype(np.int16) - np.int16(1)
    return np.select([kind == 0, kind == 1, kind == 2], [full, ext, small], tiny).astype(np.int16)


def _tiles_mix(w, h, seed):
    """m_Y / m_C: a third 0, a third 255, a third random; m_I random bytes"""
    t = (splitmix64(seed, 0, w * h * 2) & np.uint64(255)).astype(np.uint8).reshape(-1, 512)
    r = splitmix64(seed + 1, 0, t.shape[0] * 384)
    kind = r % np.uint64(3)
    pix = np.select([kind == 0, kind == 1], [np.uint64(0), np.uint64(255)], (r >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)
    t[:, :384] = pix.reshape(-1, 384)
    return t.ravel()


def _coefficients(n_regions, seed):
    """_res_mix with an all-zero region where there is more than one"""
    x = _res_mix(n_regions * 1024, seed).reshape(n_regions, 1024)
    if n_regions > 1:
        x[1] = 0
    return x


def _levels(n_regions, seed):
    """_res_mix plus the levels that reach the dequantiser's clip: the largest a forward call emits and the int16 extremes"""
    x = _res_mix(n_regions * 1024, seed).reshape(n_regions, 1024)
    x[:, 3:11] = np.array([13108, -13108, 32767, -32767, -32768, 13107, -13107, 0], np.int16)
    return x


def _bytes(n, seed, mask):
    return (splitmix64(seed, 0, n) & np.uint64(mask)).astype(np.uint8)
