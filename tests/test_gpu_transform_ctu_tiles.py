"""GPU (-m gpu): the mixed transform set per CTU straight from and into tiled frames of any size that is a multiple of 16
(xTransformCtuFromTilesDev / xTransformCtuToTilesDev).  Each 64x64 CTU is six 32x32 regions (Y0 Y1 Y2 Y3 U V), each cut into
blocks of the class its byte names.  The reference statement is numpy over the oracle: conv_input_fmt and _planes for the tile
layout, transform_fwd / transform_inv / dct32_fwd / dct32_inv per class, transform_matrix_passes for installed matrices and
np.clip for the reconstruction."""
import numpy as np
import pytest

import x266_amd
from _dev import dev
from _quant_ref import _planes, _tiles_mix
from _util import me_frames, splitmix64

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
EXTREMES = np.array([32767, -32767, -32768, 255, -255, 256, -256, 0], np.int16)
E = -1                                                                    # X266HIP_EINVAL


def _ctus(w, h):
    return (w + 63) // 64, (h + 63) // 64


def _count(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


# ---- numpy statement ----------------------------------------------------------------------------------------------------------
def _regions_of_planes(y, u, v, w, h):
    """[n_ctus, 6, 32, 32] int16 regions of three int16 planes, zero outside the frame"""
    nx, ny = _ctus(w, h)
    py = np.zeros((64 * ny, 64 * nx), np.int16)
    pu, pv = np.zeros((32 * ny, 32 * nx), np.int16), np.zeros((32 * ny, 32 * nx), np.int16)
    py[:h, :w], pu[:h // 2, :w // 2], pv[:h // 2, :w // 2] = y, u, v
    out = np.empty((ny, nx, 6, 32, 32), np.int16)
    out[:, :, :4] = py.reshape(ny, 2, 32, nx, 2, 32).transpose(0, 3, 1, 4, 2, 5).reshape(ny, nx, 4, 32, 32)
    out[:, :, 4] = pu.reshape(ny, 32, nx, 32).transpose(0, 2, 1, 3)
    out[:, :, 5] = pv.reshape(ny, 32, nx, 32).transpose(0, 2, 1, 3)
    return out.reshape(-1, 6, 32, 32)


def _planes_of_regions(reg, w, h):
    """the inverse of _regions_of_planes, cropped to the frame"""
    nx, ny = _ctus(w, h)
    r = np.asarray(reg).reshape(ny, nx, 6, 32, 32)
    y = r[:, :, :4].reshape(ny, nx, 2, 2, 32, 32).transpose(0, 2, 4, 1, 3, 5).reshape(64 * ny, 64 * nx)
    u = r[:, :, 4].transpose(0, 2, 1, 3).reshape(32 * ny, 32 * nx)
    v = r[:, :, 5].transpose(0, 2, 1, 3).reshape(32 * ny, 32 * nx)
    return y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2]


def _to_blocks(reg, n):
    """[k, 32, 32] -> [k, 1024]: (32/n)^2 blocks of n x n, block-major, blocks in raster order"""
    p = 32 // n
    return np.asarray(reg).reshape(-1, p, n, p, n).transpose(0, 1, 3, 2, 4).reshape(-1, 1024)


def _from_blocks(x, n):
    p = 32 // n
    return np.asarray(x).reshape(-1, p, p, n, n).transpose(0, 1, 3, 2, 4).reshape(-1, 32, 32)


def _slot_mats(codec):
    return {(s, n): codec.get_transform_matrix(s, n).astype(np.int16) for s in (0, 1) for n in (4, 8, 16)}


def _class_transform(oracle, k, x, inverse, mats):
    """x [m, 1024] tiles of class byte k (block-major) -> transformed; mats None: the oracle's built-in set"""
    ttype, n = (k & 15) >> 2, 4 << (k & 3)
    if n == 32:                                                           # size 32 is the 32-point DCT-II whatever the type
        return (oracle.dct32_inv if inverse else oracle.dct32_fwd)(x).reshape(-1, 1024)
    if mats is None:
        return (oracle.transform_inv if inverse else oracle.transform_fwd)(ttype, n, x).reshape(-1, 1024)
    hs, vs = int(ttype in (1, 2)), int(ttype in (1, 3))
    return oracle.transform_matrix_passes(mats[(hs, n)], mats[(vs, n)], x, inverse=inverse).reshape(-1, 1024)


def _per_class(oracle, tiles, classes, inverse, mats):
    """[m, 1024] tiles, m class bytes -> every tile transformed by its class"""
    out = np.empty_like(tiles)
    for k in np.unique(classes & 15):
        sel = (classes & 15) == k
        out[sel] = _class_transform(oracle, int(k), tiles[sel], inverse, mats)
    return out


def _ctu_residual(cur, pred, w, h, classes):
    """the CTU-ordered residual cur - pred: [n_ctus * 6, 1024] int16, zero outside the frame, block-major per region class"""
    cy, cu, cv = _planes(cur, w, h)
    py, pu, pv = _planes(pred, w, h)
    d = lambda a, b: a.astype(np.int16) - b.astype(np.int16)
    reg = _regions_of_planes(d(cy, py), d(cu, pu), d(cv, pv), w, h).reshape(-1, 32, 32)
    out = np.empty((reg.shape[0], 1024), np.int16)
    for l in range(4):
        sel = (classes & 3) == l
        out[sel] = _to_blocks(reg[sel], 4 << l)
    return out


def ref_forward(oracle, cur, pred, w, h, classes, mats=None):
    cls = np.asarray(classes, np.uint8).ravel()
    return _per_class(oracle, _ctu_residual(cur, pred, w, h, cls), cls, False, mats).reshape(-1, 6, 1024)


def _recon_of_residual(oracle, res_tiles, classes, pred, base, w, h):
    reg = np.empty((res_tiles.shape[0], 32, 32), np.int16)
    for l in range(4):
        sel = (classes & 3) == l
        reg[sel] = _from_blocks(res_tiles[sel], 4 << l)
    ry, ru, rv = _planes_of_regions(reg, w, h)
    py, pu, pv = _planes(pred, w, h)
    clip = lambda p, r: np.clip(p.astype(np.int32) + r.astype(np.int32), 0, 255).astype(np.uint8)
    packed = oracle.conv_input_fmt(clip(py, ry), clip(pu, ru), clip(pv, rv)).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    out[:, :384] = packed[:, :384]
    return out.ravel()


def ref_inverse(oracle, coef, classes, pred, w, h, base, mats=None):
    """the tile array d_recon holds after the inverse call: m_Y / m_C reconstructed, everything else as in `base`"""
    cls = np.asarray(classes, np.uint8).ravel()
    res = _per_class(oracle, np.asarray(coef, np.int16).reshape(-1, 1024), cls, True, mats)
    return _recon_of_residual(oracle, res, cls, pred, base, w, h)


# ---- data ---------------------------------------------------------------------------------------------------------------------
def _coef_mix(n, seed):
    """int16 coefficients: a quarter each full range, the extremes, small (-256..255) and -1 / 0 / 1"""
    r = splitmix64(seed, 0, n)
    kind = r & np.uint64(3)
    full = (r >> np.uint64(16)).astype(np.uint16).view(np.int16)
    ext = EXTREMES[((r >> np.uint64(48)) % np.uint64(len(EXTREMES))).astype(np.int64)]
    small = ((r >> np.uint64(32)) & np.uint64(0x1FF)).astype(np.int16) - np.int16(256)
    tiny = ((r >> np.uint64(40)) % np.uint64(3)).astype(np.int16) - np.int16(1)
    return np.select([kind == 0, kind == 1, kind == 2], [full, ext, small], tiny).astype(np.int16)


def _classes(n_ctus, seed):
    return (splitmix64(seed, 0, 6 * n_ctus) & np.uint64(15)).astype(np.uint8)


def _encoder_classes(w, h, seed):
    """mixed classes, with those an encoder uses on cut regions: luma N <= 16 on 16-row / 16-column strips, chroma N <= 16 on
    16-row strips and N <= 8 on 8- and 24-row strips (in-frame extents of the chroma region)"""
    nx, ny = _ctus(w, h)
    cls = _classes(nx * ny, seed).reshape(ny, nx, 6)
    size = cls & 3
    for q in range(4):
        ext_x = np.clip(w - (np.arange(nx) * 64 + (q & 1) * 32), 0, 32)[None, :]
        ext_y = np.clip(h - (np.arange(ny) * 64 + (q >> 1) * 32), 0, 32)[:, None]
        cut = (ext_x == 16) | (ext_y == 16)
        size[:, :, q] = np.where(cut, np.minimum(size[:, :, q], 2), size[:, :, q])
    cx = np.clip(w // 2 - np.arange(nx) * 32, 0, 32)[None, :]
    cy = np.clip(h // 2 - np.arange(ny) * 32, 0, 32)[:, None]
    lim = np.full((ny, nx), 3)
    lim = np.where((cx == 16) | (cy == 16), np.minimum(lim, 2), lim)
    lim = np.where((cx % 16 == 8) | (cy % 16 == 8), np.minimum(lim, 1), lim)
    for q in (4, 5):
        size[:, :, q] = np.minimum(size[:, :, q], lim)
    return ((cls & 12) | size).astype(np.uint8).ravel()


def _run_forward(codec, cur, pred, w, h, classes):
    n = _count(w, h)
    dc, dp, dk = dev(codec, cur), dev(codec, pred), dev(codec, classes)
    dz = dev(codec, np.full(n * 12288, SENTINEL, np.uint8))
    codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
    codec.stream_sync()
    return dz.download(np.int16, n * 6144).reshape(n, 6, 1024)


def _run_inverse(codec, coef, classes, pred, w, h, base):
    dz, dk, dp, dr = dev(codec, coef), dev(codec, classes), dev(codec, pred), dev(codec, base)
    codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    return dr.download(np.uint8, base.size)


def _wholly_outside(w, h):
    """[n_ctus, 6] bool: regions with no sample in the frame"""
    nx, ny = _ctus(w, h)
    out = np.zeros((ny, nx, 6), bool)
    for q in range(4):
        ox = (np.arange(nx) * 64 + (q & 1) * 32 >= w)[None, :]
        oy = (np.arange(ny) * 64 + (q >> 1) * 32 >= h)[:, None]
        out[:, :, q] = ox | oy
    return out.reshape(-1, 6)


# ---- 1. frame sizes and edges, 2. data extremes ---------------------------------------------------------------------------------
SIZES = [(16, 16), (48, 16), (208, 144), (80, 208), (1936, 1104), (3840, 2160), (7680, 4320)]


@pytest.mark.parametrize("w,h", SIZES)
def test_forward_and_inverse_against_numpy(codec, oracle, w, h):
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 10 + w), _tiles_mix(w, h, 20 + h)
    cls = _classes(n, 30 + w + h)
    got = _run_forward(codec, cur, pred, w, h, cls)
    assert np.array_equal(got, ref_forward(oracle, cur, pred, w, h, cls))
    outside = _wholly_outside(w, h)
    assert not got[outside].any()
    coef = _coef_mix(n * 6144, 40 + w).reshape(n, 6, 1024)
    base = np.full(pred.size, SENTINEL, np.uint8)                        # m_I must keep the sentinel
    assert np.array_equal(_run_inverse(codec, coef, cls, pred, w, h, base), ref_inverse(oracle, coef, cls, pred, w, h, base))
    # d_recon == d_pred: the same m_Y / m_C, pred's m_I kept
    dz, dk, dp = dev(codec, coef), dev(codec, cls), dev(codec, pred)
    codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dp.ptr)
    codec.stream_sync()
    assert np.array_equal(dp.download(np.uint8, pred.size), ref_inverse(oracle, coef, cls, pred, w, h, pred))


@pytest.mark.parametrize("k", range(16))
def test_every_class_byte_uniformly(codec, oracle, k):
    w, h = 208, 144
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 50 + k), _tiles_mix(w, h, 60 + k)
    cls = np.full(6 * n, k, np.uint8)
    got = _run_forward(codec, cur, pred, w, h, cls)
    assert np.array_equal(got, ref_forward(oracle, cur, pred, w, h, cls))
    assert not got[_wholly_outside(w, h)].any()
    coef = _coef_mix(n * 6144, 70 + k).reshape(n, 6, 1024)
    assert np.array_equal(_run_inverse(codec, coef, cls, pred, w, h, pred), ref_inverse(oracle, coef, cls, pred, w, h, pred))


def test_class_bytes_use_the_low_four_bits(codec, oracle):
    """the high nibble is ignored, as xTransformTilesDev ignores it"""
    w, h = 80, 208
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 81), _tiles_mix(w, h, 82)
    cls = _classes(n, 83)
    high = (cls | (splitmix64(84, 0, cls.size) & np.uint64(0xF0)).astype(np.uint8)).astype(np.uint8)
    assert np.array_equal(_run_forward(codec, cur, pred, w, h, high), _run_forward(codec, cur, pred, w, h, cls))


@pytest.mark.parametrize("fill", [0, 255])
def test_flat_pixels_and_flat_pred(codec, oracle, fill):
    """cur all 0 / 255 against a random pred and the other way round: the 9-bit residual extremes"""
    w, h = 208, 144
    n = _count(w, h)
    flat = np.full(w * h * 2, fill, np.uint8)
    rnd = _tiles_mix(w, h, 90 + fill)
    cls = _classes(n, 91 + fill)
    for cur, pred in ((flat, rnd), (rnd, flat)):
        assert np.array_equal(_run_forward(codec, cur, pred, w, h, cls), ref_forward(oracle, cur, pred, w, h, cls))
    for coef in (np.full((n, 6, 1024), 32767, np.int16), np.full((n, 6, 1024), -32768, np.int16)):
        assert np.array_equal(_run_inverse(codec, coef, cls, rnd, w, h, rnd), ref_inverse(oracle, coef, cls, rnd, w, h, rnd))


# ---- 3. equivalences on the GPU -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(208, 144), (1936, 1104)])
def test_equals_the_tile_transform_on_the_ctu_residual(codec, oracle, w, h):
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 100 + w), _tiles_mix(w, h, 101 + h)
    cls = _classes(n, 102)
    res = _ctu_residual(cur, pred, w, h, cls)
    dr, dk, dt = dev(codec, res), dev(codec, cls), codec.alloc(res.nbytes)
    codec.transform_tiles_dev(0, dr.ptr, dt.ptr, 6 * n, 0, dk.ptr)
    codec.stream_sync()
    want = dt.download(np.int16, res.size).reshape(n, 6, 1024)
    assert np.array_equal(_run_forward(codec, cur, pred, w, h, cls), want)
    # inverse = xTransformTilesDev(1) followed by the numpy reconstruction
    coef = _coef_mix(n * 6144, 103)
    dz = dev(codec, coef)
    codec.transform_tiles_dev(1, dz.ptr, dt.ptr, 6 * n, 0, dk.ptr)
    codec.stream_sync()
    res_back = dt.download(np.int16, coef.size).reshape(-1, 1024)
    want_tiles = _recon_of_residual(oracle, res_back, cls, pred, pred, w, h)
    assert np.array_equal(_run_inverse(codec, coef, cls, pred, w, h, pred), want_tiles)


@pytest.mark.parametrize("w,h", [(64, 64), (320, 192), (3840, 2176)])
def test_all_dct32_equals_the_dct32_ctu_calls(codec, w, h):
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 110 + w), _tiles_mix(w, h, 111 + h)
    cls = np.full(6 * n, 3, np.uint8)                                    # X266_TILE_CLASS(X266_TR_DCT2, 32)
    dc, dp, dk = dev(codec, cur), dev(codec, pred), dev(codec, cls)
    dz = codec.alloc(n * 12288)
    codec.dct32_fwd_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dz.ptr)
    codec.stream_sync()
    want = dz.download(np.int16, n * 6144).reshape(n, 6, 1024)
    assert np.array_equal(_run_forward(codec, cur, pred, w, h, cls), want)
    coef = _coef_mix(n * 6144, 112)
    dz.upload(coef)
    dr = dev(codec, np.full(pred.size, SENTINEL, np.uint8))
    codec.dct32_inv_ctu_to_tiles_dev(dz.ptr, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    base = np.full(pred.size, SENTINEL, np.uint8)
    assert np.array_equal(_run_inverse(codec, coef, cls, pred, w, h, base), dr.download(np.uint8, pred.size))


# ---- 4. installed matrices ----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fresh():
    """a context of its own: installed matrices are per context"""
    c = x266_amd.Codec(0)
    yield c
    c.close()


def _check_with_installed(fresh, oracle, seed):
    w, h = 208, 144
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, seed), _tiles_mix(w, h, seed + 1)
    cls = _classes(n, seed + 2)
    mats = _slot_mats(fresh)
    assert np.array_equal(_run_forward(fresh, cur, pred, w, h, cls), ref_forward(oracle, cur, pred, w, h, cls, mats))
    coef = _coef_mix(n * 6144, seed + 3).reshape(n, 6, 1024)
    assert np.array_equal(_run_inverse(fresh, coef, cls, pred, w, h, pred), ref_inverse(oracle, coef, cls, pred, w, h, pred, mats))


def test_installed_preset_dct8(fresh, oracle):
    fresh.use_transform_preset(2)                                        # X266_PRESET_VTM_DCT8
    try:
        _check_with_installed(fresh, oracle, 120)
    finally:
        fresh.use_transform_preset(0)


def test_installed_random_int8_matrices(fresh, oracle):
    rng = np.random.default_rng(130)
    try:
        for s in (0, 1):
            for n in (4, 8, 16):
                m = rng.integers(-128, 128, (n, n)).astype(np.int8)
                m.flat[0], m.flat[-1] = -128, 127
                fresh.set_transform_matrix(s, n, m)
        _check_with_installed(fresh, oracle, 131)
    finally:
        for s in (0, 1):
            for n in (4, 8, 16):
                fresh.set_transform_matrix(s, n, None)


# ---- 5. frames over 4 GiB ----------------------------------------------------------------------------------------------------------
def test_frames_beyond_4_gib(codec, oracle):
    """A 65536 x 33040 frame (4.3 GB per tile array, 6.5 GB of coefficients, the last CTU row cut to 16 rows), filled on the device:
    the CTUs at the start, on each side of the 2^32-byte boundary of the tile arrays and of the coefficient stream, and at the end"""
    w, h = 65536, 33040
    tiles_x, nt = w // 16, (w // 16) * (h // 16)
    nx, ny = _ctus(w, h)
    n = nx * ny
    assert nt * 512 > (1 << 32) and n * 12288 > (1 << 32)
    d_cur, d_pred, d_coef = codec.alloc(nt * 512), codec.alloc(nt * 512), codec.alloc(n * 12288)
    codec.fill_residual_dev(d_cur.ptr, nt * 256, 0xC0)                  # any bytes are a valid tile array
    codec.fill_residual_dev(d_pred.ptr, nt * 256, 0xC1)
    cls = _classes(n, 0xC2)
    d_cls = dev(codec, cls)

    def fetch(buf, byte_off, count, dtype):
        out = np.empty(count, dtype)
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, out.ctypes.data, buf.ptr + byte_off, out.nbytes), "D2H")
        return out

    def ctu_tiles(buf, cy, cx):
        """the CTU's in-frame tiles as a small frame of its own"""
        tw, th = min(4, tiles_x - 4 * cx), min(4, h // 16 - 4 * cy)
        rows = [fetch(buf, ((4 * cy + j) * tiles_x + 4 * cx) * 512, tw * 512, np.uint8) for j in range(th)]
        return np.concatenate(rows), 16 * tw, 16 * th

    t_edge = (1 << 32) // 512
    c_edge = (1 << 32) // 12288
    picks = {0, ((t_edge // tiles_x) // 4) * nx + (t_edge % tiles_x) // 4, (((t_edge - 1) // tiles_x) // 4) * nx + ((t_edge - 1) % tiles_x) // 4,
             c_edge, c_edge + 1, n - nx, n - 1}
    pred_before = {b: ctu_tiles(d_pred, b // nx, b % nx) for b in picks}
    codec.transform_ctu_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, d_cls.ptr, d_coef.ptr)
    codec.transform_ctu_to_tiles_dev(d_coef.ptr, d_cls.ptr, d_pred.ptr, w, h, d_pred.ptr)      # in place
    codec.stream_sync()
    for b in sorted(picks):
        cy, cx = b // nx, b % nx
        cur, cw, chh = ctu_tiles(d_cur, cy, cx)
        pred = pred_before[b][0]
        k = cls[6 * b:6 * b + 6]
        coef = fetch(d_coef, b * 12288, 6144, np.int16).reshape(1, 6, 1024)
        assert np.array_equal(coef, ref_forward(oracle, cur, pred, cw, chh, k)), b
        got, _, _ = ctu_tiles(d_pred, cy, cx)
        assert np.array_equal(got, ref_inverse(oracle, coef, k, pred, cw, chh, pred)), b


# ---- 6. the inter loop at 2160p ---------------------------------------------------------------------------------------------------
def test_inter_loop_at_2160p_and_in_a_graph(codec, oracle):
    """search from tiles -> MC -> forward CTU call with an encoder-like class map -> inverse CTU call over the prediction; the
    transform stages against the oracle on the GPU's own pred, then the same sequence captured once and replayed"""
    w, h, rng = 3840, 2160, 8
    n = _count(w, h)
    cur_y, ref_y = me_frames(w, h, 0, 1400, mv=(5, -3), noise=4)
    r = splitmix64(1401, 0, w * h)
    u, v = (r[: w * h // 4] & np.uint64(255)).astype(np.uint8), ((r[w * h // 4:w * h // 2] >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)
    cur = oracle.conv_input_fmt(cur_y, u.reshape(h // 2, w // 2), v.reshape(h // 2, w // 2))
    ref = oracle.conv_input_fmt(ref_y, np.roll(u, 7).reshape(h // 2, w // 2), np.roll(v, 11).reshape(h // 2, w // 2))
    cls = _encoder_classes(w, h, 1402)
    assert set(np.unique(cls[6 * (n - 1) + 2:6 * (n - 1) + 4] & 3)) <= {0, 1, 2}
    nb = (w // 8) * (h // 8)
    dc, dr, dk = dev(codec, cur), dev(codec, ref), dev(codec, cls)
    db, dp, dz = codec.alloc(nb * 8), dev(codec, ref), codec.alloc(n * 12288)  # pred starts as the reference: co-located chroma
    st = codec.stream_create()
    try:
        codec._check(codec.L.xHipMeScratchReserve(codec.ctx, st, w, h), "xHipMeScratchReserve")

        def enqueue():
            codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr, stream=st)
            codec.motion_comp_luma_dev(dr.ptr, db.ptr, w, h, dp.ptr, stream=st)
            codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr, stream=st)
            codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dp.ptr, stream=st)

        def results():
            codec.stream_sync(st)
            return db.download(np.uint8, nb * 8), dz.download(np.int16, n * 6144), dp.download(np.uint8, w * h * 2)

        # eager, stage by stage: the GPU's own pred is the oracle's input
        codec.satd_search_from_tiles_dev(dc.ptr, dr.ptr, w, h, rng, db.ptr, stream=st)
        codec.motion_comp_luma_dev(dr.ptr, db.ptr, w, h, dp.ptr, stream=st)
        codec.stream_sync(st)
        pred = dp.download(np.uint8, w * h * 2)
        assert np.array_equal(pred.reshape(-1, 512)[:, 256:], ref.reshape(-1, 512)[:, 256:])   # MC writes only m_Y
        codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr, stream=st)
        codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dp.ptr, stream=st)
        eager = results()
        coef = eager[1].reshape(n, 6, 1024)
        assert np.array_equal(coef, ref_forward(oracle, cur, pred, w, h, cls))
        assert np.array_equal(eager[2], ref_inverse(oracle, coef, cls, pred, w, h, pred))

        dp.upload(ref)
        codec.graph_begin(st)
        enqueue()
        graph = codec.graph_end(st)
        try:
            for _ in range(2):
                db.upload(np.zeros(nb * 8, np.uint8))
                dz.upload(np.zeros(n * 12288, np.uint8))
                dp.upload(ref)
                codec.graph_launch(graph, st)
                for a, b in zip(eager, results()):
                    assert np.array_equal(a, b)
        finally:
            codec.graph_free(graph)
    finally:
        codec.stream_destroy(st)


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(codec, oracle):
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(1 << 22)
    p = buf.ptr
    c, r, z, k, o = p, p + (1 << 20), p + (2 << 20), p + (3 << 20), p + (3 << 20) + (1 << 19)   # cur, pred, coef, classes, recon
    codec.stream_sync()
    fwd = lambda *a: L.xTransformCtuFromTilesDev(ctx, *a, None)
    inv = lambda *a: L.xTransformCtuToTilesDev(ctx, *a, None)
    for wh in ((0, 64), (64, 0), (-16, 64), (64, -16), (24, 64), (64, 40), (8, 16)):
        assert fwd(c, r, wh[0], wh[1], k, z) == E, wh
        assert inv(z, k, r, wh[0], wh[1], o) == E, wh
    # NULL buffers
    assert fwd(None, r, 64, 64, k, z) == E and fwd(c, None, 64, 64, k, z) == E
    assert fwd(c, r, 64, 64, None, z) == E and fwd(c, r, 64, 64, k, None) == E
    assert inv(None, k, r, 64, 64, o) == E and inv(z, None, r, 64, 64, o) == E
    assert inv(z, k, None, 64, 64, o) == E and inv(z, k, r, 64, 64, None) == E
    # alignment: tiles and coefficients 16 bytes, classes any
    for off in (1, 8):
        assert fwd(c + off, r, 64, 64, k, z) == E and fwd(c, r + off, 64, 64, k, z) == E and fwd(c, r, 64, 64, k, z + off) == E
        assert inv(z + off, k, r, 64, 64, o) == E and inv(z, k, r + off, 64, 64, o) == E and inv(z, k, r, 64, 64, o + off) == E
    # overlaps: the forward output with each input (an 80x80 frame: 4 CTUs, 49152 bytes of coefficients, 12800 bytes of tiles)
    assert fwd(c, r, 80, 80, k, c + 4096) == E and fwd(c, r, 80, 80, k, r - 16384) == E
    assert fwd(c, r, 80, 80, k, k - 49152 + 16) == E
    assert fwd(c, c, 80, 80, k, z) == 0                                  # d_cur == d_pred: both read-only
    # overlaps of the inverse output: with pred (partial), coefficients, classes; d_recon == d_pred is allowed
    assert inv(z, k, r, 80, 80, r + 512) == E and inv(z, k, r, 80, 80, r - 512) == E
    assert inv(z, k, r, 80, 80, z + 49152 - 16) == E and inv(z, k, r, 80, 80, k - 12800 + 16) == E
    assert inv(z, k, r, 80, 80, r) == 0
    # spans that would run past the end of the address space
    top = (1 << 64) - 4096
    assert fwd(c, r, 64, 64, k, top) == E and inv(z, k, r, 64, 64, top) == E
    assert fwd(top, r, 64, 64, k, z) == E and inv(top, k, r, 64, 64, o) == E
    assert fwd(c, r, 64, 64, (1 << 64) - 2, z) == E
    codec.stream_sync()
    # a class table at an odd address reads the same bytes
    w, h = 80, 80
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 140), _tiles_mix(w, h, 141)
    cls = _classes(n, 142)
    raw = np.zeros(6 * n + 3, np.uint8)
    raw[3:] = cls
    dc, dp, dk, dz = dev(codec, cur), dev(codec, pred), dev(codec, raw), codec.alloc(n * 12288)
    codec.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr + 3, dz.ptr)
    codec.stream_sync()
    coef = dz.download(np.int16, n * 6144).reshape(n, 6, 1024)
    assert np.array_equal(coef, ref_forward(oracle, cur, pred, w, h, cls))
    dr = dev(codec, pred)
    codec.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr + 3, dp.ptr, w, h, dr.ptr)
    codec.stream_sync()
    assert np.array_equal(dr.download(np.uint8, pred.size), ref_inverse(oracle, coef, cls, pred, w, h, pred))


# ---- the numpy conveniences ----------------------------------------------------------------------------------------------------------
def test_host_conveniences_round_trip(codec, oracle):
    w, h = 48, 16
    n = _count(w, h)
    cur, pred = _tiles_mix(w, h, 150), _tiles_mix(w, h, 151)
    cls = _classes(n, 152)
    coef = codec.transform_ctu_from_tiles(cur, pred, w, h, cls)
    assert coef.shape == (n, 6, 1024) and np.array_equal(coef, ref_forward(oracle, cur, pred, w, h, cls))
    rec = codec.transform_ctu_to_tiles(coef, cls, pred, w, h)
    assert np.array_equal(rec, ref_inverse(oracle, coef, cls, pred, w, h, pred))
