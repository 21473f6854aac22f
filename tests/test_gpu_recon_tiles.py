"""GPU (-m gpu): reconstruction into tiled frames -- recon = clip8(pred + residual) written into m_Y / m_C of ref_block_t tiles
(src/x266.cpp:56-63), unfused (xReconLumaDev, xReconChromaDev) and fused with the inverse DCT32 (xDct32InvToTilesDev,
xDct32InvCtuToTilesDev).  The reference statement is numpy over the oracle: oracle.conv_input_fmt for the tile layout,
oracle.dct32_inv / residual_luma / residual_chroma, plus np.clip."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from _dev import dev
from _quant_ref import _clip, _planes
from _util import extremes_np, fullrange_np, residual_np, splitmix64

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
EXTREMES = np.array([32767, -32767, -32768, 255, -255, 256, -256], np.int16)


# ---- numpy statement of the tile layout and of the reconstruction ---------------------------------------------------------
def _unblocks(b, hh, ww, edge):
    return np.asarray(b).reshape(hh // edge, ww // edge, edge, edge).transpose(0, 2, 1, 3).reshape(hh, ww)


def _with(oracle, base, w, h, y=None, u=None, v=None):
    """`base` tiles with m_Y (y given) and / or m_C (u, v given) replaced by the oracle's packing of those planes"""
    py, pu, pv = _planes(base, w, h)
    packed = oracle.conv_input_fmt(py if y is None else y, pu if u is None else u, pv if v is None else v).reshape(-1, 512)
    out = np.array(base, np.uint8).reshape(-1, 512)
    if y is not None:
        out[:, :256] = packed[:, :256]
    if u is not None:
        out[:, 256:384] = packed[:, 256:384]
    return out.ravel()


# ---- data ---------------------------------------------------------------------------------------------------------------------
def _res_mix(n, seed):
    """int16 residuals: a quarter each full range, the extremes of EXTREMES, small (-256..255) and +-1 / 0"""
    r = splitmix64(seed, 0, n)
    kind = r & np.uint64(3)
    full = (r >> np.uint64(16)).astype(np.uint16).view(np.int16)
    ext = EXTREMES[((r >> np.uint64(48)) % np.uint64(len(EXTREMES))).astype(np.int64)]
    small = ((r >> np.uint64(32)) & np.uint64(0x1FF)).astype(np.int16) - np.int16(256)
    tiny = ((r >> np.uint64(40)) % np.uint64(3)).astype(np.int16) - np.int16(1)
    return np.select([kind == 0, kind == 1, kind == 2], [full, ext, small], tiny).astype(np.int16)


def _pix_mix(n, seed):
    """pixels: a third 0, a third 255, a third random"""
    r = splitmix64(seed, 0, n)
    kind = r % np.uint64(3)
    return np.select([kind == 0, kind == 1], [np.uint64(0), np.uint64(255)], (r >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)


def _tiles_mix(w, h, seed):
    """a tile array whose m_Y / m_C samples are _pix_mix and whose m_I holds random bytes"""
    t = (splitmix64(seed, 0, w * h * 2) & np.uint64(255)).astype(np.uint8).reshape(-1, 512)
    t[:, :384] = _pix_mix(t.shape[0] * 384, seed + 1).reshape(-1, 384)
    return t.ravel()


def _assert_pairs_covered(pred, res):
    """every extreme residual meets pred 0 and pred 255 somewhere in the data"""
    p, r = pred.ravel(), res.ravel()
    for v in EXTREMES:
        for q in (0, 255):
            assert np.any((r == v) & (p == q)), (int(v), q)


def _sentinel(codec, nbytes):
    return dev(codec, np.full(nbytes, SENTINEL, np.uint8))


# ---- 1. unfused reconstruction against numpy, 5. in place ----------------------------------------------------------------------
@pytest.mark.parametrize("edge,w,h", [(8, 48, 16), (8, 208, 112), (8, 3840, 2160), (32, 224, 416), (32, 64, 32), (32, 1920, 1088)])
def test_recon_luma_against_numpy(codec, oracle, edge, w, h):
    pred = _tiles_mix(w, h, 100 + w + edge)
    res = _res_mix(w * h, 200 + h + edge)
    py, _, _ = _planes(pred, w, h)
    plane = _unblocks(res.reshape(-1, edge * edge), h, w, edge)
    _assert_pairs_covered(py, plane)
    want_y = _clip(py, plane)
    d_pred, d_res = dev(codec, pred), dev(codec, res)
    d_out = _sentinel(codec, pred.nbytes)                                # m_C and m_I must keep the sentinel
    codec.recon_luma_dev(d_pred.ptr, d_res.ptr, w, h, edge, d_out.ptr)
    codec.stream_sync()
    got = d_out.download(np.uint8, pred.nbytes)
    assert np.array_equal(got, _with(oracle, np.full(pred.size, SENTINEL, np.uint8), w, h, y=want_y))
    assert np.array_equal(d_pred.download(np.uint8, pred.nbytes), pred)  # the input is not touched
    d_inplace = dev(codec, pred)                                         # d_recon == d_pred: same m_Y, the rest of pred kept
    codec.recon_luma_dev(d_inplace.ptr, d_res.ptr, w, h, edge, d_inplace.ptr)
    codec.stream_sync()
    assert np.array_equal(d_inplace.download(np.uint8, pred.nbytes), _with(oracle, pred, w, h, y=want_y))


@pytest.mark.parametrize("edge,w,h", [(8, 48, 16), (8, 208, 112), (8, 3840, 2160), (32, 320, 192), (32, 64, 64), (32, 1920, 1024)])
@pytest.mark.parametrize("pitch", [1, 2, 3])
def test_recon_chroma_against_numpy(codec, oracle, edge, w, h, pitch):
    pred = _tiles_mix(w, h, 300 + w + edge)
    _, pu, pv = _planes(pred, w, h)
    npl = (w // 2) * (h // 2)
    n = npl // (edge * edge)
    res_u, res_v = _res_mix(npl, 400 + h + edge), _res_mix(npl, 500 + h + edge)
    plane_u, plane_v = _unblocks(res_u, h // 2, w // 2, edge), _unblocks(res_v, h // 2, w // 2, edge)
    _assert_pairs_covered(np.concatenate([pu.ravel(), pv.ravel()]), np.concatenate([plane_u.ravel(), plane_v.ravel()]))
    want_u, want_v = _clip(pu, plane_u), _clip(pv, plane_v)
    if pitch == 1:                                                       # two planar block streams
        d_u, d_v = dev(codec, res_u), dev(codec, res_v)
        pu_ptr, pv_ptr = d_u.ptr, d_v.ptr
    else:                                                                # one stream U0 V0 (hole) U1 V1 (hole) ...
        both = np.full((n, pitch, edge * edge), 0x7777, np.int16)
        both[:, 0], both[:, 1] = res_u.reshape(n, -1), res_v.reshape(n, -1)
        d_both = dev(codec, both)
        pu_ptr, pv_ptr = d_both.ptr, d_both.ptr + edge * edge * 2
    d_pred = dev(codec, pred)
    d_out = _sentinel(codec, pred.nbytes)                                # m_Y and m_I must keep the sentinel
    codec.recon_chroma_dev(d_pred.ptr, pu_ptr, pv_ptr, w, h, edge, d_out.ptr, pitch)
    codec.stream_sync()
    got = d_out.download(np.uint8, pred.nbytes)
    assert np.array_equal(got, _with(oracle, np.full(pred.size, SENTINEL, np.uint8), w, h, u=want_u, v=want_v))
    d_inplace = dev(codec, pred)
    codec.recon_chroma_dev(d_inplace.ptr, pu_ptr, pv_ptr, w, h, edge, d_inplace.ptr, pitch)
    codec.stream_sync()
    assert np.array_equal(d_inplace.download(np.uint8, pred.nbytes), _with(oracle, pred, w, h, u=want_u, v=want_v))


# ---- 2. round trip: residual of (cur, pred), reconstructed onto pred, is cur ------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 64), (320, 192), (208, 112), (1920, 1088)])
def test_residual_then_recon_gives_back_cur(codec, oracle, w, h):
    cur, pred = _tiles_mix(w, h, 600 + w), _tiles_mix(w, h, 700 + w)
    cy, cu, cv = _planes(cur, w, h)
    d_cur = dev(codec, cur)
    npl = (w // 2) * (h // 2)
    for ledge in ((32, 8) if w % 32 == 0 and h % 32 == 0 else (8,)):
        for cedge in ((32, 8) if w % 64 == 0 and h % 64 == 0 else (8,)):
            d_pred = dev(codec, pred)
            d_res, d_ru, d_rv = codec.alloc(w * h * 2), codec.alloc(npl * 2), codec.alloc(npl * 2)
            codec.residual_luma_dev(d_cur.ptr, d_pred.ptr, w, h, ledge, d_res.ptr)
            codec.residual_chroma_dev(d_cur.ptr, d_pred.ptr, w, h, cedge, d_ru.ptr, d_rv.ptr)
            codec.stream_sync()
            assert np.array_equal(d_res.download(np.int16, w * h), oracle.residual_luma(cur, pred, w, h, ledge))
            codec.recon_luma_dev(d_pred.ptr, d_res.ptr, w, h, ledge, d_pred.ptr)              # onto pred, in place
            codec.stream_sync()
            assert np.array_equal(d_pred.download(np.uint8, cur.nbytes), _with(oracle, pred, w, h, y=cy))
            codec.recon_chroma_dev(d_pred.ptr, d_ru.ptr, d_rv.ptr, w, h, cedge, d_pred.ptr)   # composes with the luma call
            codec.stream_sync()
            got = d_pred.download(np.uint8, cur.nbytes).reshape(-1, 512)
            assert np.array_equal(got[:, :384], cur.reshape(-1, 512)[:, :384]), (ledge, cedge)
            assert np.array_equal(got[:, 384:], pred.reshape(-1, 512)[:, 384:])                 # m_I of pred, untouched
            oy, ou, ov = codec.alloc(w * h), codec.alloc(npl), codec.alloc(npl)
            codec.conv_output_420_dev(d_pred.ptr, oy.ptr, w, ou.ptr, ov.ptr, w // 2, w, h)
            codec.stream_sync()
            assert np.array_equal(oy.download(np.uint8, w * h).reshape(h, w), cy)
            assert np.array_equal(ou.download(np.uint8, npl).reshape(h // 2, w // 2), cu)
            assert np.array_equal(ov.download(np.uint8, npl).reshape(h // 2, w // 2), cv)


# ---- 3. fused luma --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(32, 32), (96, 64), (224, 416), (1920, 1088)])
@pytest.mark.parametrize("source", ["fullrange", "forward"])
def test_fused_inverse_into_tiles(codec, oracle, w, h, source):
    """xDct32InvToTilesDev == xDct32InvBatchDev + xReconLumaDev(.., 32, ..) == clip(pred + oracle.dct32_inv(coef)), every block;
    on full-range coefficients (the inverse's int16 clipping) and on xDct32FwdFromTilesDev's (the real loop)"""
    n = (w // 32) * (h // 32)
    pred = _tiles_mix(w, h, 800 + w)
    d_pred = dev(codec, pred)
    if source == "fullrange":
        coef = fullrange_np(n * 1024, 900 + w).reshape(n, 1024)
        d_coef = dev(codec, coef)
    else:
        d_cur = dev(codec, _tiles_mix(w, h, 901 + w))
        d_coef = codec.alloc(n * 2048)
        codec.dct32_fwd_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, d_coef.ptr)
        codec.stream_sync()
        coef = d_coef.download(np.int16, n * 1024).reshape(n, 1024)
    res = oracle.dct32_inv(coef, threads=8)
    py, _, _ = _planes(pred, w, h)
    want = _with(oracle, pred, w, h, y=_clip(py, _unblocks(res, h, w, 32)))
    # two-call path
    d_res, d_two = codec.alloc(n * 2048), dev(codec, pred)
    codec.dct32_inv_dev(d_coef.ptr, d_res.ptr, n)
    codec.recon_luma_dev(d_two.ptr, d_res.ptr, w, h, 32, d_two.ptr)
    codec.stream_sync()
    assert np.array_equal(d_res.download(np.int16, n * 1024).reshape(n, 1024), res)
    two = d_two.download(np.uint8, pred.nbytes)
    assert np.array_equal(two, want)
    # fused, out of place (sentinel: m_C and m_I untouched) and in place
    d_out = _sentinel(codec, pred.nbytes)
    codec.dct32_inv_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_out.ptr)
    codec.stream_sync()
    got = d_out.download(np.uint8, pred.nbytes).reshape(-1, 512)
    assert np.array_equal(got[:, :256], want.reshape(-1, 512)[:, :256])
    assert np.all(got[:, 256:] == SENTINEL)
    codec.dct32_inv_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_pred.ptr)
    codec.stream_sync()
    assert np.array_equal(d_pred.download(np.uint8, pred.nbytes), two)


def test_fused_inverse_follows_the_inverse_blocks_per_wave_option(codec, oracle):
    """the fused kernel runs in the inverse batch's launch shape: every blocks-per-wave setting gives the same bytes"""
    w, h = 416, 224
    n = (w // 32) * (h // 32)
    pred = _tiles_mix(w, h, 1000)
    coef = extremes_np(n * 1024, 1001)
    d_pred, d_coef = dev(codec, pred), dev(codec, coef)
    py, _, _ = _planes(pred, w, h)
    want = _with(oracle, pred, w, h, y=_clip(py, _unblocks(oracle.dct32_inv(coef, threads=8), h, w, 32)))
    saved, adaptive = codec.get_option("dct32_inv_blocks_per_wave"), codec.get_option("adaptive_per_wave")
    try:
        codec.set_option("adaptive_per_wave", 0)                            # or 91 blocks run one per wave whatever the option says (tests/_option_cases.py)
        for bpw in (1, 2, 3, 7):
            codec.set_option("dct32_inv_blocks_per_wave", bpw)
            d_out = dev(codec, pred)
            codec.dct32_inv_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_out.ptr)
            codec.stream_sync()
            assert np.array_equal(d_out.download(np.uint8, pred.nbytes), want), bpw
    finally:
        codec.set_option("dct32_inv_blocks_per_wave", saved)
        codec.set_option("adaptive_per_wave", adaptive)


# ---- 4. whole CTU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 64), (320, 192), (3840, 2176)])
@pytest.mark.parametrize("source", ["forward", "fullrange"])
def test_whole_ctu_inverse_into_tiles(codec, oracle, w, h, source):
    """xDct32FwdCtuFromTilesDev -> xDct32InvCtuToTilesDev == the six blocks' inverse + the unfused luma and chroma recon calls,
    on whole tiles, m_I untouched"""
    n_ctu = (w // 64) * (h // 64)
    cur, pred = _tiles_mix(w, h, 1100 + w), _tiles_mix(w, h, 1200 + w)
    d_cur, d_pred = dev(codec, cur), dev(codec, pred)
    if source == "forward":
        d_coef = codec.alloc(n_ctu * 12288)
        codec.dct32_fwd_ctu_from_tiles_dev(d_cur.ptr, d_pred.ptr, w, h, d_coef.ptr)
        codec.stream_sync()
        coef = d_coef.download(np.int16, n_ctu * 6144)
    else:
        coef = fullrange_np(n_ctu * 6144, 1300 + w)
        d_coef = dev(codec, coef)
    # unfused: the inverse batch of all six blocks, luma re-ordered to frame raster, chroma read in place at block_pitch 6
    d_res = codec.alloc(n_ctu * 12288)
    codec.dct32_inv_dev(d_coef.ptr, d_res.ptr, n_ctu * 6)
    codec.stream_sync()
    res = d_res.download(np.int16, n_ctu * 6144).reshape(n_ctu, 6, 1024)
    assert np.array_equal(res.reshape(-1, 1024), oracle.dct32_inv(coef, threads=8))
    luma = res[:, :4].reshape(h // 64, w // 64, 2, 2, 1024).transpose(0, 2, 1, 3, 4).reshape(-1)
    d_luma, d_two = dev(codec, luma), _sentinel(codec, cur.nbytes)
    codec.recon_luma_dev(d_pred.ptr, d_luma.ptr, w, h, 32, d_two.ptr)
    codec.recon_chroma_dev(d_pred.ptr, d_res.ptr + 4 * 2048, d_res.ptr + 5 * 2048, w, h, 32, d_two.ptr, 6)
    codec.stream_sync()
    two = d_two.download(np.uint8, cur.nbytes)
    py, pu, pv = _planes(pred, w, h)
    want_y = _clip(py, _unblocks(luma, h, w, 32))
    want_u, want_v = _clip(pu, _unblocks(res[:, 4], h // 2, w // 2, 32)), _clip(pv, _unblocks(res[:, 5], h // 2, w // 2, 32))
    assert np.array_equal(two, _with(oracle, np.full(cur.size, SENTINEL, np.uint8), w, h, y=want_y, u=want_u, v=want_v))
    # fused, out of place and in place
    d_out = _sentinel(codec, cur.nbytes)
    codec.dct32_inv_ctu_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_out.ptr)
    codec.stream_sync()
    assert np.array_equal(d_out.download(np.uint8, cur.nbytes), two)
    codec.dct32_inv_ctu_to_tiles_dev(d_coef.ptr, d_pred.ptr, w, h, d_pred.ptr)
    codec.stream_sync()
    assert np.array_equal(d_pred.download(np.uint8, cur.nbytes), _with(oracle, pred, w, h, y=want_y, u=want_u, v=want_v))


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors(codec):
    L, ctx = codec.L, codec.ctx
    buf = codec.alloc(1 << 22)
    p = buf.ptr
    t, r = p, p + (1 << 20)                                              # a 64x64 tile array (8 KiB) and a residual / coefficient area
    o = p + (2 << 20)                                                    # a second tile array
    E = -1                                                               # X266HIP_EINVAL
    # luma: edge, frame size, NULL, alignment, overlaps
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 16, o, None) == E
    assert L.xReconLumaDev(ctx, t, r, 48, 32, 32, o, None) == E         # 48 % 32
    assert L.xReconLumaDev(ctx, t, r, 24, 16, 8, o, None) == E          # 24 % 16
    assert L.xReconLumaDev(ctx, t, r, 0, 16, 8, o, None) == E
    assert L.xReconLumaDev(ctx, None, r, 64, 64, 8, o, None) == E
    assert L.xReconLumaDev(ctx, t, None, 64, 64, 8, o, None) == E
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 8, None, None) == E
    assert L.xReconLumaDev(ctx, t + 8, r, 64, 64, 8, o, None) == E
    assert L.xReconLumaDev(ctx, t, r + 2, 64, 64, 8, o, None) == E
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 8, o + 4, None) == E
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 8, t + 512, None) == E    # partial overlap with pred
    assert L.xReconLumaDev(ctx, t + 512, r, 64, 64, 8, t, None) == E
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 8, r + 4096, None) == E   # recon over the residual
    assert L.xReconLumaDev(ctx, t, o + 4096, 64, 64, 8, o, None) == E   # residual inside recon
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 32, t, None) == 0         # in place
    assert L.xReconLumaDev(ctx, t, r, 64, 64, 8, o, None) == 0
    # chroma: the same, plus block_pitch 0 and a block_pitch whose span overflows size_t
    assert L.xReconChromaDev(ctx, t, r, r + 8192, 1, 96, 64, 32, o, None) == E      # 96 % 64
    assert L.xReconChromaDev(ctx, t, r, r + 8192, 1, 64, 64, 16, o, None) == E      # edge
    assert L.xReconChromaDev(ctx, t, r, r + 8192, 0, 64, 64, 8, o, None) == E       # pitch 0
    # 16 blocks of 128 bytes: the span ((n - 1) * pitch + 1) * 128 must neither wrap size_t nor run past the address space
    assert L.xReconChromaDev(ctx, t, r, r + 8192, (1 << 63) // 64, 64, 64, 8, o, None) == E      # the product wraps
    assert L.xReconChromaDev(ctx, t, r, r + 8192, (1 << 64) - 1, 64, 64, 8, o, None) == E
    assert L.xReconChromaDev(ctx, t, r, r + 8192, ((1 << 64) - (1 << 20)) // (15 * 128), 64, 64, 8, o, None) == E   # r + span wraps
    assert L.xReconChromaDev(ctx, t, r, r + 8192, 1 << 62, 64, 64, 32, o, None) == 0     # one block per plane: the pitch is never applied
    assert L.xReconChromaDev(ctx, t, None, r, 1, 64, 64, 8, o, None) == E
    assert L.xReconChromaDev(ctx, t, r, r + 8, 1, 64, 64, 8, o, None) == E           # unaligned V
    assert L.xReconChromaDev(ctx, t, r, r + 8192, 1, 64, 64, 8, t + 1024, None) == E   # partial overlap with pred
    assert L.xReconChromaDev(ctx, t, o + 64, r, 1, 64, 64, 8, o, None) == E          # U inside recon
    assert L.xReconChromaDev(ctx, t, r, o + 1024, 2, 64, 64, 8, o, None) == E        # V inside recon
    assert L.xReconChromaDev(ctx, t, r, r + 128, 2, 64, 64, 8, t, None) == 0         # interleaved, in place
    assert L.xReconChromaDev(ctx, t, r, r + 2048, 2, 64, 64, 32, o, None) == 0
    # fused
    assert L.xDct32InvToTilesDev(ctx, r, t, 48, 32, o, None) == E
    assert L.xDct32InvToTilesDev(ctx, None, t, 64, 64, o, None) == E
    assert L.xDct32InvToTilesDev(ctx, r + 2, t, 64, 64, o, None) == E
    assert L.xDct32InvToTilesDev(ctx, r, t, 64, 64, t + 16, None) == E
    assert L.xDct32InvToTilesDev(ctx, r, t, 64, 64, r - 4096, None) == E      # recon runs into the coefficients
    assert L.xDct32InvToTilesDev(ctx, r, t, 64, 64, t, None) == 0
    assert L.xDct32InvCtuToTilesDev(ctx, r, t, 96, 64, o, None) == E
    assert L.xDct32InvCtuToTilesDev(ctx, r, t, 64, 32, o, None) == E
    assert L.xDct32InvCtuToTilesDev(ctx, r, None, 64, 64, o, None) == E
    assert L.xDct32InvCtuToTilesDev(ctx, r, t + 8, 64, 64, o, None) == E
    assert L.xDct32InvCtuToTilesDev(ctx, r, t, 64, 64, t + 512, None) == E
    assert L.xDct32InvCtuToTilesDev(ctx, r, t, 64, 64, r + 8192, None) == E   # recon over the CTU's 12 KiB of coefficients
    assert L.xDct32InvCtuToTilesDev(ctx, r, t, 64, 64, o, None) == 0
    codec.stream_sync()


# ---- 6. beyond 4 GiB -----------------------------------------------------------------------------------------------------------------
def test_recon_of_tile_frames_beyond_4_gib(codec, oracle):
    """A 65568 x 32768 frame (8 392 704 tiles = 4.3 GB per tile array, 4.3 GB of residual): 32x32 regions at the start, around the
    tile whose byte offset is 2^32 and at the frame's far corners -- xReconLumaDev in both block orders, xDct32InvToTilesDev."""
    w, h = 65536 + 32, 32768
    tiles_x, nt = w // 16, (w // 16) * (h // 16)
    assert nt * 512 > (1 << 32) and w * h > (1 << 31)
    d_pred, d_res = codec.alloc(nt * 512), codec.alloc(w * h * 2)
    codec.fill_residual_dev(d_pred.ptr, nt * 256, 0xD0)                 # any bytes are a valid tile array
    codec.fill_residual_dev(d_res.ptr, w * h, 0xD1)                     # read as 32x32 blocks, as 8x8 blocks, and as coefficients
    d_r32, d_r8, d_fused = codec.alloc(nt * 512), codec.alloc(nt * 512), codec.alloc(nt * 512)
    codec.recon_luma_dev(d_pred.ptr, d_res.ptr, w, h, 32, d_r32.ptr)
    codec.recon_luma_dev(d_pred.ptr, d_res.ptr, w, h, 8, d_r8.ptr)
    codec.dct32_inv_to_tiles_dev(d_res.ptr, d_pred.ptr, w, h, d_fused.ptr)
    codec.stream_sync()

    def fetch(buf, byte_off, count, dtype):
        out = np.empty(count, dtype)
        codec._check(codec.L.xHipMemcpyD2H(codec.ctx, out.ctypes.data, buf.ptr + byte_off, out.nbytes), "D2H")
        return out

    t_edge = (1 << 32) // 512
    regions = [(0, 0), (t_edge // tiles_x // 2, (t_edge % tiles_x) // 2), (h // 32 - 1, w // 32 - 1), (h // 32 - 1, 0), (h // 64, w // 32 - 1)]
    for by, bx in regions:
        four = lambda buf: np.concatenate([fetch(buf, ((2 * by + j) * tiles_x + 2 * bx) * 512, 1024, np.uint8) for j in (0, 1)])
        tp = four(d_pred)
        py, _, _ = _planes(tp, 32, 32)
        blk = by * (w // 32) + bx
        r32 = fetch(d_res, blk * 2048, 1024, np.int16)
        assert np.array_equal(_planes(four(d_r32), 32, 32)[0], _clip(py, r32.reshape(32, 32))), (by, bx)
        z = oracle.dct32_inv(r32).reshape(32, 32)
        assert np.array_equal(_planes(four(d_fused), 32, 32)[0], _clip(py, z)), (by, bx)
        r8 = np.stack([fetch(d_res, ((4 * by + j) * (w // 8) + 4 * bx) * 128, 256, np.int16) for j in range(4)])
        plane8 = r8.reshape(4, 4, 8, 8).transpose(0, 2, 1, 3).reshape(32, 32)
        assert np.array_equal(_planes(four(d_r8), 32, 32)[0], _clip(py, plane8)), (by, bx)


# ---- 7. randomised ---------------------------------------------------------------------------------------------------------------
def fuzz(n):
    return settings(max_examples=n, deadline=None, derandomize=True, database=None,
                    suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow, HealthCheck.data_too_large])


@fuzz(40)
@given(cw=st.integers(1, 12), ch=st.integers(1, 8), half=st.integers(0, 1), kind=st.integers(0, 3), pitch=st.integers(1, 3),
       in_place=st.booleans(), seed=st.integers(1, 1 << 30))
def test_recon_random(codec, oracle, cw, ch, half, kind, pitch, in_place, seed):
    """random frame sizes (64x64 CTUs, or 16x16 tiles with ragged 8-tile groups when `half`), data mixes, block_pitch and
    in-place choice: every reconstruction entry point that the size admits, against numpy"""
    w, h = (cw * 16 + 16 * (seed % 5), ch * 16) if half else (cw * 64, ch * 64)
    npx = w * h
    gen = (_res_mix, fullrange_np, extremes_np, residual_np)[kind]
    pred = _tiles_mix(w, h, seed)
    py, pu, pv = _planes(pred, w, h)
    d_pred = dev(codec, pred)

    def run(call):
        d_out = dev(codec, pred) if in_place else _sentinel(codec, pred.nbytes)
        call(d_out.ptr if in_place else d_pred.ptr, d_out.ptr)
        codec.stream_sync()
        return d_out.download(np.uint8, pred.nbytes)

    base = pred if in_place else np.full(pred.size, SENTINEL, np.uint8)
    for edge in (8, 32):
        if w % (2 * edge if edge == 8 else 32) or h % (2 * edge if edge == 8 else 32):
            continue
        res = gen(npx, seed + edge)
        d_res = dev(codec, res)
        got = run(lambda src, dst: codec.recon_luma_dev(src, d_res.ptr, w, h, edge, dst))
        assert np.array_equal(got, _with(oracle, base, w, h, y=_clip(py, _unblocks(res, h, w, edge)))), edge
        if edge == 32:
            got = run(lambda src, dst: codec.dct32_inv_to_tiles_dev(d_res.ptr, src, w, h, dst))
            z = oracle.dct32_inv(res, threads=8)
            assert np.array_equal(got, _with(oracle, base, w, h, y=_clip(py, _unblocks(z, h, w, 32))))
    for edge in (8, 32):
        if w % (16 if edge == 8 else 64) or h % (16 if edge == 8 else 64):
            continue
        npl = npx // 4
        n = npl // (edge * edge)
        ru, rv = gen(npl, seed + 3 * edge), gen(npl, seed + 5 * edge)
        both = np.zeros((n, pitch, 2, edge * edge), np.int16)            # U stream and V stream each at `pitch`, V after U's holes
        both[:, 0, 0], both[:, 0, 1] = ru.reshape(n, -1), rv.reshape(n, -1)
        flat = np.concatenate([both[:, :, 0].ravel(), both[:, :, 1].ravel()])
        d_both = dev(codec, flat)
        pv_ptr = d_both.ptr + n * pitch * edge * edge * 2
        got = run(lambda src, dst: codec.recon_chroma_dev(src, d_both.ptr, pv_ptr, w, h, edge, dst, pitch))
        want = _with(oracle, base, w, h, u=_clip(pu, _unblocks(ru, h // 2, w // 2, edge)), v=_clip(pv, _unblocks(rv, h // 2, w // 2, edge)))
        assert np.array_equal(got, want), (edge, pitch)
    if w % 64 == 0 and h % 64 == 0:
        n_ctu = npx // 4096
        coef = gen(n_ctu * 6144, seed + 7)
        d_coef = dev(codec, coef)
        got = run(lambda src, dst: codec.dct32_inv_ctu_to_tiles_dev(d_coef.ptr, src, w, h, dst))
        z = oracle.dct32_inv(coef, threads=8).reshape(n_ctu, 6, 1024)
        zy = z[:, :4].reshape(h // 64, w // 64, 2, 2, 1024).transpose(0, 2, 1, 3, 4).reshape(-1, 1024)
        want = _with(oracle, base, w, h, y=_clip(py, _unblocks(zy, h, w, 32)), u=_clip(pu, _unblocks(z[:, 4], h // 2, w // 2, 32)),
                     v=_clip(pv, _unblocks(z[:, 5], h // 2, w // 2, 32)))
        assert np.array_equal(got, want)
