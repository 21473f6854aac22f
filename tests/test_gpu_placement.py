"""Every device entry point of include/x266hip.h at the MINIMUM alignment its argument check accepts, inside guard bands.

The rest of the suite hands the library pointers straight from xHipMalloc (256-byte aligned or better) and allocates nothing
behind the last output byte.  Here every pointer argument of every `...Dev` call sits in an allocation of its own
(tests/_arena.py: 64 KiB guard | displacement | payload | 64 KiB guard) at `alignment x odd` bytes, a different odd multiplier
per argument; the results are compared bit for bit with the references the family tests already use (the oracle, and the numpy
statements of test_gpu_mc_chroma / me_tiles / recon_tiles / transform_ctu_tiles), the guards and every documented hole (pitch
gaps, m_I, the plane a call does not write) must still hold the fill, and each case runs under two seeds of input-guard garbage.
The same case at natural alignment (displacement 0) makes a failure attributable to placement.  The rejection table displaces
one argument at a time by half its alignment: X266HIP_EINVAL, an error text, not one byte written.

ROWS is the table: per entry point the pointer arguments with the alignment x266_amd/csrc/x266_args.hpp enforces (1 = none), the variants
(shapes at which a tail or a per-wave run can go wrong, launch forms forced through the options), and how to build inputs,
output extents and the reference.  Two tests here need no GPU: the table covers the header's `...Dev` declarations exactly, and
every variant builds; tests/test_docs_follow_code.py checks that the header states the table's alignments."""
import collections
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from _arena import Arena
from _dev import EINVAL, records, sync_or_exit, tiles
from _util import fullrange_np, intra_refs_np, me_frames, residual_np, splitmix64
import test_gpu_mc_chroma as mcc
import test_gpu_me_tiles as met
import test_gpu_recon_tiles as rct
import test_gpu_transform_ctu_tiles as ctu

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# `...Dev(` declarations of the header that have no row.  Fixed: a new entry point needs a row, not an entry here.
EXCLUDED = frozenset()

Case = collections.namedtuple("Case", "inputs outputs call options")     # inputs {name: array | (array, origin)}; outputs {name: (want bytes, written mask | None)}
Row = collections.namedtuple("Row", "ptrs variants build")                # ptrs: ordered {name: alignment}
ROWS = collections.OrderedDict()


def row(name, ptrs, variants):
    def deco(fn):
        ROWS[name] = Row(collections.OrderedDict(ptrs), variants, fn)
        return fn
    return deco


def product(**axes):
    out = [{}]
    for k, vals in axes.items():
        out = [dict(d, **{k: v}) for d in out for v in vals]
    return out


def _b(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _mixed(n, unit, seed):
    """n units of int16: even ones with the reference's stimulus distribution, odd ones full range"""
    a = residual_np(n * unit, seed).reshape(n, unit).copy()
    a[1::2] = fullrange_np(n * unit, seed + 1).reshape(n, unit)[1::2]
    return a


def _pitched(blocks, pitch):
    """blocks [n, k] at a pitch of `pitch` blocks -> (bytes of the span, written mask): the holes are what a call must not touch"""
    blocks = np.ascontiguousarray(blocks)
    n, bb = blocks.shape[0], blocks[0].nbytes
    span = ((n - 1) * pitch + 1) * bb
    want, mask = np.zeros(span, np.uint8), np.zeros(span, bool)
    for i in range(n):
        want[i * pitch * bb:i * pitch * bb + bb] = _b(blocks[i])
        mask[i * pitch * bb:i * pitch * bb + bb] = True
    return want, mask


def _pitched_in(blocks, pitch, seed):
    """the same layout as an input: the holes hold garbage"""
    want, mask = _pitched(blocks, pitch)
    return np.where(mask, want, (splitmix64(seed, 0, want.size) & np.uint64(255)).astype(np.uint8))


def _tile_mask(n_tiles, luma, chroma):
    m = np.zeros((n_tiles, 512), bool)
    m[:, :256], m[:, 256:384] = luma, chroma                              # m_I (384..511) is never written
    return m.ravel()


# Small batches run ONE unit per wave whatever the per-wave options say ("adaptive_per_wave", default 1): the rows whose kernels loop
# over several units set it to 0, so that the loops the large batches run are the ones placed here.
LOOPS = {"adaptive_per_wave": 0}
DCT_COUNTS = [1, 2, 3, 7, 9, 17]            # 1 / 2 / 8 blocks per wave, 64- and 256-thread workgroups
SATD_COUNTS = [1, 31, 33, 255, 257, 289]    # the 32-block group and the 8-group store burst
INTRA_COUNTS = [1, 3, 4, 5, 9]              # a wave takes four blocks
FRAMES16 = [(16, 16), (48, 32), (80, 48)]   # odd tile counts
FRAMES32 = [(32, 32), (96, 64), (160, 96)]
FRAMES64 = [(64, 64), (128, 64), (192, 128)]


# ---- DCT32 family ----------------------------------------------------------------------------------------------------------------
@row("xDct32FwdBatchDev", [("d_in", 16), ("d_out", 16)],
     product(n=DCT_COUNTS, opt=[(0, 64, 1), (0, 256, 3), (2, 0, 1)]))
def _(oracle, n, opt):
    x = _mixed(n, 1024, 10 + n)
    return Case({"d_in": x}, {"d_out": (_b(oracle.dct32_fwd(x)), None)},
                lambda L, c, p: L.xDct32FwdBatchDev(c, p["d_in"], p["d_out"], n, None),
                dict(LOOPS, dct32_variant=opt[0], dct32_wg_threads=opt[1], dct32_blocks_per_wave=opt[2]))


@row("xDct32InvBatchDev", [("d_in", 16), ("d_out", 16)], product(n=DCT_COUNTS, bpw=[1, 2], wg=[64, 256]))
def _(oracle, n, bpw, wg):
    z = _mixed(n, 1024, 20 + n)
    return Case({"d_in": z}, {"d_out": (_b(oracle.dct32_inv(z)), None)},
                lambda L, c, p: L.xDct32InvBatchDev(c, p["d_in"], p["d_out"], n, None),
                dict(LOOPS, dct32_inv_blocks_per_wave=bpw, dct32_wg_threads=wg))


@row("xDct32FwdInvBatchDev", [("d_in", 16), ("d_coef", 16), ("d_recon", 16)],
     product(n=DCT_COUNTS, coef=[True, False], bpw=[0, 1, 2], wg=[64, 256]))
def _(oracle, n, coef, bpw, wg):
    x = _mixed(n, 1024, 30 + n)
    z = oracle.dct32_fwd(x)
    outs = {"d_recon": (_b(oracle.dct32_inv(z)), None)}
    if coef:
        outs["d_coef"] = (_b(z), None)
    return Case({"d_in": x}, outs, lambda L, c, p: L.xDct32FwdInvBatchDev(c, p["d_in"], p["d_coef"], p["d_recon"], n, None),
                dict(LOOPS, dct32_fwdinv_blocks_per_wave=bpw, dct32_wg_threads=wg))    # bpw 0 = automatic: 2, and 8 without d_coef


@row("xDct32PassDev", [("d_in", 16), ("d_out", 16)], product(n=DCT_COUNTS, shift=[4, 11]))
def _(oracle, n, shift):
    x = _mixed(n, 1024, 40 + n)
    want = np.stack([oracle.dct32_pass(x[b], shift) for b in range(n)])
    return Case({"d_in": x}, {"d_out": (_b(want), None)},
                lambda L, c, p: L.xDct32PassDev(c, p["d_in"], p["d_out"], n, shift, None), {})


@row("xDct32SatdFrameDev", [("d_dct_in", 16), ("d_dct_out", 16), ("d_diff", 16), ("d_satd_out", 16)],
     product(n=[(1, 31), (2, 33), (3, 255), (7, 257), (9, 289), (17, 1)], satd_variant=[0, 1, 3]) +        # the run length left at 0
     product(n=[(1, 31), (2, 33), (3, 255), (7, 257), (9, 289), (17, 1)], satd_variant=[0, 1, 3], gpw=[1, 3]))
def _(oracle, n, satd_variant, gpw=0):
    nd, ns = n
    x, d = _mixed(nd, 1024, 50 + nd), _mixed(ns, 64, 51 + ns)
    return Case({"d_dct_in": x, "d_diff": d},
                {"d_dct_out": (_b(oracle.dct32_fwd(x)), None), "d_satd_out": (_b(oracle.satd8x8(d)), None)},
                lambda L, c, p: L.xDct32SatdFrameDev(c, p["d_dct_in"], p["d_dct_out"], nd, p["d_diff"], p["d_satd_out"], ns, None),
                dict(LOOPS, satd_variant=satd_variant, satd_groups_per_wave=gpw))   # the lanes' run length: 0 = 2, the staged body's default


# ---- SATD / SAD batches ------------------------------------------------------------------------------------------------------------
@row("xSatd8x8BatchDev", [("d_diff", 16), ("d_out", 4)], product(n=SATD_COUNTS, satd_variant=[0, 1, 2, 3], gpw=[0, 8, 1]))
def _(oracle, n, satd_variant, gpw):
    d = _mixed(n, 64, 60 + n)
    return Case({"d_diff": d}, {"d_out": (_b(oracle.satd8x8(d)), None)},
                lambda L, c, p: L.xSatd8x8BatchDev(c, p["d_diff"], p["d_out"], n, None),
                dict(LOOPS, satd_variant=satd_variant, satd_groups_per_wave=gpw))    # 8 groups: the LDS-DMA kernel's whole store burst


def _sad_counts(edge):
    unit = max(4096 // (edge * edge), 1)                                  # blocks in 256 chunks of 16 bytes: a wave's run (4 x 4: four waves')
    return sorted({c for c in (1, unit // 4 - 1, unit // 4 + 1, unit - 1, unit, unit + 1, 2 * unit + 1, 4 * unit + 1) if c > 0})   # ... and a second workgroup


@row("xSadBatchDev", [("d_a", 16), ("d_b", 16), ("d_out", 4)],
     [dict(edge=e, n=n) for e in (4, 8, 16, 32, 64) for n in _sad_counts(e)])
def _(oracle, edge, n):
    r = splitmix64(70 + edge + n, 0, 2 * n * edge * edge)
    a = (r[:n * edge * edge] & np.uint64(255)).astype(np.uint8).reshape(n, -1)
    b = ((r[n * edge * edge:] >> np.uint64(9)) & np.uint64(255)).astype(np.uint8).reshape(n, -1)
    a[0], b[0] = 255, 0                                                  # the largest sum
    want = np.abs(a.astype(np.int64) - b.astype(np.int64)).sum(axis=1).astype(np.uint32)
    return Case({"d_a": a, "d_b": b}, {"d_out": (_b(want), None)},
                lambda L, c, p: L.xSadBatchDev(c, edge, p["d_a"], p["d_b"], p["d_out"], n, None), {})


# ---- the transform set -------------------------------------------------------------------------------------------------------------
def _set_counts(size):
    per_tile = (32 // size) ** 2
    return sorted({c for c in (1, per_tile - 1, per_tile + 1, 2 * per_tile + 3) if c > 0})


SET_VARIANTS = [dict(cls=(t, s), n=n, offsets=o, wg=wg) for t, s in ((0, 4), (1, 8), (3, 16), (0, 32)) for n in _set_counts(s)
                for o in (False, True) for wg in (64, 256)]


def _set_case(oracle, entry, inverse, cls, n, offsets, wg):
    ttype, size = cls
    unit = size * size
    x = _mixed(n, unit, 80 + size + n + inverse)
    if size == 32:
        y = (oracle.dct32_inv if inverse else oracle.dct32_fwd)(x)
    else:
        y = (oracle.transform_inv if inverse else oracle.transform_fwd)(ttype, size, x)
    ins = {}
    if offsets:                                                           # the blocks scattered over a buffer with three spare slots
        order = np.random.default_rng(n + size).permutation(n + 3)[:n]
        src = fullrange_np((n + 3) * unit, 81).reshape(n + 3, unit).copy()
        want, mask = np.zeros((n + 3, unit), np.int16), np.zeros((n + 3, unit), bool)
        src[order], want[order], mask[order] = x, y, True
        ins["d_offsets"] = (order * unit).astype(np.uint32)
        x, y, written = src, want, np.repeat(mask.ravel(), 2)
    else:
        written = None
    ins["d_in"] = x
    return Case(ins, {"d_out": (_b(y), written)},
                lambda L, c, p: getattr(L, entry)(c, ttype, size, p["d_in"], p["d_out"], n, p["d_offsets"], None),
                dict(LOOPS, dct32_wg_threads=wg))


@row("xTransformFwdBatchDev", [("d_in", 16), ("d_out", 16), ("d_offsets", 4)], SET_VARIANTS)
def _(oracle, cls, n, offsets, wg):
    return _set_case(oracle, "xTransformFwdBatchDev", 0, cls, n, offsets, wg)


@row("xTransformInvBatchDev", [("d_in", 16), ("d_out", 16), ("d_offsets", 4)], SET_VARIANTS)
def _(oracle, cls, n, offsets, wg):
    return _set_case(oracle, "xTransformInvBatchDev", 1, cls, n, offsets, wg)


TILE_CLASSES = [(0, 4), (0, 8), (0, 16), (0, 32), (1, 4), (1, 8), (1, 16), (2, 4), (2, 8), (2, 16), (3, 4), (3, 8), (3, 16)]


def _tile_transform(oracle, tiles, classes, inverse):
    """[n, 1024] block-major tiles, one class byte each -> every tile transformed by its class"""
    return ctu._per_class(oracle, tiles, classes, bool(inverse), None)


@row("xTransformTilesDev", [("d_in", 16), ("d_out", 16), ("d_tile_offsets", 4), ("d_tile_class", 1)],
     product(inverse=[0, 1], n=[1, 2, 3, 4, 7], offsets=[False, True], tpw=[1, 3]))
def _(oracle, inverse, n, offsets, tpw):
    pick = np.random.default_rng(90 + n).integers(0, len(TILE_CLASSES), n)
    classes = np.array([TILE_CLASSES[k][0] * 4 + {4: 0, 8: 1, 16: 2, 32: 3}[TILE_CLASSES[k][1]] for k in pick], np.uint8)
    x = _mixed(n, 1024, 91 + n + inverse)
    y = _tile_transform(oracle, x, classes, inverse)
    ins = {"d_tile_class": classes}
    written = None
    if offsets:
        order = np.random.default_rng(92 + n).permutation(n + 2)[:n]
        src = fullrange_np((n + 2) * 1024, 93).reshape(n + 2, 1024).copy()
        want, mask = np.zeros((n + 2, 1024), np.int16), np.zeros((n + 2, 1024), bool)
        src[order], want[order], mask[order] = x, y, True
        ins["d_tile_offsets"] = (order * 1024).astype(np.uint32)
        x, y, written = src, want, np.repeat(mask.ravel(), 2)
    ins["d_in"] = x
    return Case(ins, {"d_out": (_b(y), written)},
                lambda L, c, p: L.xTransformTilesDev(c, inverse, p["d_in"], p["d_out"], n, p["d_tile_offsets"], p["d_tile_class"], None),
                dict(LOOPS, tile_tiles_per_wave=tpw))


# ---- tiled frames: packing, residuals, the fused forms -------------------------------------------------------------------------------
def _yuv(w, h, seed):
    r = splitmix64(seed, 0, w * h * 3 // 2)
    p = (r & np.uint64(255)).astype(np.uint8)
    return p[:w * h].reshape(h, w), p[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), p[w * h * 5 // 4:].reshape(h // 2, w // 2)


def _strided(plane, stride, seed):
    """the plane's rows `stride` bytes apart, garbage in the gaps, no gap after the last row -> (bytes, mask of the plane's bytes)"""
    h, w = plane.shape
    buf = (splitmix64(seed, 0, h * stride) & np.uint64(255)).astype(np.uint8).reshape(h, stride)
    mask = np.zeros((h, stride), bool)
    buf[:, :w], mask[:, :w] = plane, True
    return buf.ravel()[:(h - 1) * stride + w].copy(), mask.ravel()[:(h - 1) * stride + w].copy()


@row("xConvInputFmtDev", [("d_tiles", 16), ("d_y", 16), ("d_u", 8), ("d_v", 8)], product(size=FRAMES16, gap=[0, 16]))
def _(oracle, size, gap):
    w, h = size
    y, u, v = _yuv(w, h, 100 + w)
    strd = w + gap
    want = oracle.conv_input_fmt(y, u, v)
    return Case({"d_y": _strided(y, strd, 1)[0], "d_u": _strided(u, strd // 2, 2)[0], "d_v": _strided(v, strd // 2, 3)[0]},
                {"d_tiles": (want, _tile_mask(want.size // 512, True, True))},
                lambda L, c, p: L.xConvInputFmtDev(c, p["d_tiles"], p["d_y"], p["d_u"], p["d_v"], strd, w, h, None), {})


@row("xConvOutput420Dev", [("d_tiles", 16), ("d_y", 16), ("d_u", 8), ("d_v", 8)], product(size=FRAMES16, gap=[0, 16]))
def _(oracle, size, gap):
    w, h = size
    tiles = rct._tiles_mix(w, h, 110 + w)
    y, u, v = oracle.conv_output_420(tiles, w, h)
    strd_y, strd_c = w + gap, w // 2 + gap // 2
    return Case({"d_tiles": tiles}, {"d_y": _strided(y, strd_y, 1), "d_u": _strided(u, strd_c, 2), "d_v": _strided(v, strd_c, 3)},
                lambda L, c, p: L.xConvOutput420Dev(c, p["d_tiles"], p["d_y"], strd_y, p["d_u"], p["d_v"], strd_c, w, h, None), {})


def _two_frames(w, h, seed):
    return rct._tiles_mix(w, h, seed), rct._tiles_mix(w, h, seed + 7)


@row("xResidualLumaDev", [("d_cur", 16), ("d_pred", 16), ("d_residual", 16)],
     [dict(edge=8, size=s) for s in FRAMES16] + [dict(edge=32, size=s) for s in FRAMES32])
def _(oracle, edge, size):
    w, h = size
    cur, pred = _two_frames(w, h, 120 + w)
    return Case({"d_cur": cur, "d_pred": pred}, {"d_residual": (_b(oracle.residual_luma(cur, pred, w, h, edge)), None)},
                lambda L, c, p: L.xResidualLumaDev(c, p["d_cur"], p["d_pred"], w, h, edge, p["d_residual"], None), {})


@row("xDct32FwdFromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_coef", 16)], product(size=FRAMES32, wg=[64, 256]))
def _(oracle, size, wg):
    w, h = size
    cur, pred = _two_frames(w, h, 130 + w)
    want = oracle.dct32_fwd(oracle.residual_luma(cur, pred, w, h, 32))
    return Case({"d_cur": cur, "d_pred": pred}, {"d_coef": (_b(want), None)},
                lambda L, c, p: L.xDct32FwdFromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_coef"], None), {"dct32_wg_threads": wg})


@row("xSatd8x8FromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_out", 4)],
     product(size=FRAMES16 + [(272, 64)], satd_variant=[0, 1, 3]))          # 272 x 64: 272 blocks, eight and a half groups
def _(oracle, size, satd_variant):
    w, h = size
    cur, pred = _two_frames(w, h, 140 + w)
    want = oracle.satd8x8(oracle.residual_luma(cur, pred, w, h, 8))
    return Case({"d_cur": cur, "d_pred": pred}, {"d_out": (_b(want), None)},
                lambda L, c, p: L.xSatd8x8FromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_out"], None), {"satd_variant": satd_variant})


@row("xResidualChromaDev", [("d_cur", 16), ("d_pred", 16), ("d_res_u", 16), ("d_res_v", 16)],
     [dict(edge=8, size=s, pitch=q) for s in FRAMES16 for q in (1, 2)] + [dict(edge=32, size=s, pitch=q) for s in FRAMES64 for q in (1, 2)])
def _(oracle, edge, size, pitch):
    w, h = size
    cur, pred = _two_frames(w, h, 150 + w)
    ru, rv = oracle.residual_chroma(cur, pred, w, h, edge)
    return Case({"d_cur": cur, "d_pred": pred},
                {"d_res_u": _pitched(ru.reshape(-1, edge * edge), pitch), "d_res_v": _pitched(rv.reshape(-1, edge * edge), pitch)},
                lambda L, c, p: L.xResidualChromaDev(c, p["d_cur"], p["d_pred"], w, h, edge, p["d_res_u"], p["d_res_v"], pitch, None), {})


@row("xDct32FwdChromaFromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_coef_u", 16), ("d_coef_v", 16)],
     product(size=FRAMES64, pitch=[1, 2], wg=[64, 256]))
def _(oracle, size, pitch, wg):
    w, h = size
    cur, pred = _two_frames(w, h, 160 + w)
    ru, rv = oracle.residual_chroma(cur, pred, w, h, 32)
    return Case({"d_cur": cur, "d_pred": pred},
                {"d_coef_u": _pitched(oracle.dct32_fwd(ru), pitch), "d_coef_v": _pitched(oracle.dct32_fwd(rv), pitch)},
                lambda L, c, p: L.xDct32FwdChromaFromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_coef_u"], p["d_coef_v"], pitch, None),
                {"dct32_wg_threads": wg})


def _all_dct32(w, h):
    return np.full(6 * ctu._count(w, h), 3, np.uint8)                    # X266_TILE_CLASS(DCT-II, 32) for every region


@row("xDct32FwdCtuFromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_coef", 16)], product(size=FRAMES64, wg=[64, 256]))
def _(oracle, size, wg):
    w, h = size
    cur, pred = _two_frames(w, h, 170 + w)
    want = ctu.ref_forward(oracle, cur, pred, w, h, _all_dct32(w, h))
    return Case({"d_cur": cur, "d_pred": pred}, {"d_coef": (_b(want), None)},
                lambda L, c, p: L.xDct32FwdCtuFromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_coef"], None), {"dct32_wg_threads": wg})


@row("xSatd8x8ChromaFromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_out_u", 4), ("d_out_v", 4)],
     product(size=FRAMES16 + [(272, 64)], pitch=[1, 2]))
def _(oracle, size, pitch):
    w, h = size
    cur, pred = _two_frames(w, h, 180 + w)
    ru, rv = oracle.residual_chroma(cur, pred, w, h, 8)
    return Case({"d_cur": cur, "d_pred": pred},
                {"d_out_u": _pitched(oracle.satd8x8(ru).reshape(-1, 1), pitch), "d_out_v": _pitched(oracle.satd8x8(rv).reshape(-1, 1), pitch)},
                lambda L, c, p: L.xSatd8x8ChromaFromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_out_u"], p["d_out_v"], pitch, None), {})


# ---- reconstruction into tiles ---------------------------------------------------------------------------------------------------
def _recon_want(oracle, pred, w, h, y=None, u=None, v=None):
    """(bytes, mask): the planes given replace pred's; only their bytes are written"""
    n_tiles = pred.size // 512
    return rct._with(oracle, pred, w, h, y=y, u=u, v=v), _tile_mask(n_tiles, y is not None, u is not None)


@row("xReconLumaDev", [("d_pred", 16), ("d_residual", 16), ("d_recon", 16)],
     [dict(edge=8, size=s) for s in FRAMES16] + [dict(edge=32, size=s) for s in FRAMES32])
def _(oracle, edge, size):
    w, h = size
    pred, res = rct._tiles_mix(w, h, 190 + w), rct._res_mix(w * h, 191 + w)
    py, _, _ = rct._planes(pred, w, h)
    want = rct._clip(py, rct._unblocks(res.reshape(-1, edge * edge), h, w, edge))
    return Case({"d_pred": pred, "d_residual": res}, {"d_recon": _recon_want(oracle, pred, w, h, y=want)},
                lambda L, c, p: L.xReconLumaDev(c, p["d_pred"], p["d_residual"], w, h, edge, p["d_recon"], None), {})


@row("xReconChromaDev", [("d_pred", 16), ("d_res_u", 16), ("d_res_v", 16), ("d_recon", 16)],
     [dict(edge=8, size=s, pitch=q) for s in FRAMES16 for q in (1, 2)] + [dict(edge=32, size=s, pitch=q) for s in FRAMES64 for q in (1, 2)])
def _(oracle, edge, size, pitch):
    w, h = size
    npl = (w // 2) * (h // 2)
    pred, ru, rv = rct._tiles_mix(w, h, 200 + w), rct._res_mix(npl, 201 + w), rct._res_mix(npl, 202 + w)
    _, pu, pv = rct._planes(pred, w, h)
    want_u = rct._clip(pu, rct._unblocks(ru, h // 2, w // 2, edge))
    want_v = rct._clip(pv, rct._unblocks(rv, h // 2, w // 2, edge))
    return Case({"d_pred": pred, "d_res_u": _pitched_in(ru.reshape(-1, edge * edge), pitch, 5), "d_res_v": _pitched_in(rv.reshape(-1, edge * edge), pitch, 6)},
                {"d_recon": _recon_want(oracle, pred, w, h, u=want_u, v=want_v)},
                lambda L, c, p: L.xReconChromaDev(c, p["d_pred"], p["d_res_u"], p["d_res_v"], pitch, w, h, edge, p["d_recon"], None), {})


@row("xDct32InvToTilesDev", [("d_coef", 16), ("d_pred", 16), ("d_recon", 16)], product(size=FRAMES32, opt=[(1, 64), (2, 256), (3, 64)]))
def _(oracle, size, opt):
    w, h = size
    n = (w // 32) * (h // 32)
    pred, coef = rct._tiles_mix(w, h, 210 + w), _mixed(n, 1024, 211 + w)
    py, _, _ = rct._planes(pred, w, h)
    want = rct._clip(py, rct._unblocks(oracle.dct32_inv(coef), h, w, 32))
    return Case({"d_coef": coef, "d_pred": pred}, {"d_recon": _recon_want(oracle, pred, w, h, y=want)},
                lambda L, c, p: L.xDct32InvToTilesDev(c, p["d_coef"], p["d_pred"], w, h, p["d_recon"], None),
                dict(LOOPS, dct32_inv_blocks_per_wave=opt[0], dct32_wg_threads=opt[1]))


def _ctu_inverse_want(oracle, coef, classes, pred, w, h):
    return ctu.ref_inverse(oracle, coef, classes, pred, w, h, pred), _tile_mask(pred.size // 512, True, True)


@row("xDct32InvCtuToTilesDev", [("d_coef", 16), ("d_pred", 16), ("d_recon", 16)], product(size=FRAMES64, wg=[64, 256]))
def _(oracle, size, wg):
    w, h = size
    pred, coef = rct._tiles_mix(w, h, 220 + w), _mixed(6 * ctu._count(w, h), 1024, 221 + w)
    return Case({"d_coef": coef, "d_pred": pred}, {"d_recon": _ctu_inverse_want(oracle, coef, _all_dct32(w, h), pred, w, h)},
                lambda L, c, p: L.xDct32InvCtuToTilesDev(c, p["d_coef"], p["d_pred"], w, h, p["d_recon"], None), {"dct32_wg_threads": wg})


# ---- the mixed transform set per CTU, cut CTUs included ---------------------------------------------------------------------------
CTU_FRAMES = [(80, 48), (64, 64), (144, 80)]


@row("xTransformCtuFromTilesDev", [("d_cur", 16), ("d_pred", 16), ("d_class", 1), ("d_coef", 16)], product(size=CTU_FRAMES, wg=[64, 256]))
def _(oracle, size, wg):
    w, h = size
    cur, pred = ctu._tiles_mix(w, h, 230 + w), ctu._tiles_mix(w, h, 231 + w)
    classes = ctu._encoder_classes(w, h, 232 + w)
    want = ctu.ref_forward(oracle, cur, pred, w, h, classes)
    return Case({"d_cur": cur, "d_pred": pred, "d_class": classes}, {"d_coef": (_b(want), None)},
                lambda L, c, p: L.xTransformCtuFromTilesDev(c, p["d_cur"], p["d_pred"], w, h, p["d_class"], p["d_coef"], None),
                {"dct32_wg_threads": wg})


@row("xTransformCtuToTilesDev", [("d_coef", 16), ("d_class", 1), ("d_pred", 16), ("d_recon", 16)], product(size=CTU_FRAMES, wg=[64, 256]))
def _(oracle, size, wg):
    w, h = size
    pred, coef = ctu._tiles_mix(w, h, 240 + w), ctu._coef_mix(6144 * ctu._count(w, h), 241 + w)
    classes = ctu._encoder_classes(w, h, 242 + w)
    return Case({"d_coef": coef, "d_class": classes, "d_pred": pred}, {"d_recon": _ctu_inverse_want(oracle, coef, classes, pred, w, h)},
                lambda L, c, p: L.xTransformCtuToTilesDev(c, p["d_coef"], p["d_class"], p["d_pred"], w, h, p["d_recon"], None),
                {"dct32_wg_threads": wg})


# ---- motion search and compensation ----------------------------------------------------------------------------------------------------
RANGE, PAD = 3, 4                             # 49-entry cost maps; a border of 4 keeps the origin's offset inside the frame even


def _best_records(mv, cost):
    rec = np.zeros((len(mv), 4), np.int16)
    rec[:, :2] = mv
    rec.view(np.uint32)[:, 1] = cost
    return rec


def _search_outputs(oracle, cur, refp, pad, metric, costs):
    mv, cost, cmap = oracle.satd_search(cur, refp, pad, RANGE, want_costs=True, metric=metric)
    outs = {"d_best": (_b(_best_records(mv, cost)), None)}
    if costs:
        outs["d_costs"] = (_b(cmap), None)
    return outs


def _planar_search(oracle, entry, metric, size, costs, rows, gap):
    """gap: rows further apart than they have to be, by the smallest step the call accepts (SATD: any stride; SAD: cur_stride a multiple of 4)"""
    w, h = size
    cur, refp = me_frames(w, h, PAD, 250 + w, mv=(2, -1))
    cur_stride, ref_stride = w + gap * (3 if metric == "satd" else 4), w + 2 * PAD + gap
    return Case({"d_cur": _strided(cur, cur_stride, 4)[0], "d_ref": (_strided(refp, ref_stride, 5)[0], PAD * ref_stride + PAD)},
                _search_outputs(oracle, cur, refp, PAD, metric, costs),
                lambda L, c, p: getattr(L, entry)(c, p["d_cur"], cur_stride, p["d_ref"], ref_stride, w, h, RANGE, p["d_best"], p["d_costs"], None),
                {"me_tile_rows": rows})


PLANAR = product(size=[(16, 16), (40, 24)], costs=[True, False], rows=[1, 0], gap=[0, 1])


@row("xSatd8x8SearchDev", [("d_cur", 1), ("d_ref", 1), ("d_best", 8), ("d_costs", 4)], PLANAR)
def _(oracle, size, costs, rows, gap):
    return _planar_search(oracle, "xSatd8x8SearchDev", "satd", size, costs, rows, gap)


@row("xSad8x8SearchDev", [("d_cur", 4), ("d_ref", 1), ("d_best", 8), ("d_costs", 4)], PLANAR)
def _(oracle, size, costs, rows, gap):
    return _planar_search(oracle, "xSad8x8SearchDev", "sad", size, costs, rows, gap)


def _tiled_search(oracle, entry, metric, size, costs, rows):
    w, h = size
    cur, ref = me_frames(w, h, 0, 260 + w, mv=(2, -1))
    ct, rt = met._tiles(oracle, cur, 261), met._tiles(oracle, ref, 262)
    return Case({"d_cur": ct, "d_ref": rt}, _search_outputs(oracle, cur, np.pad(ref, RANGE, mode="edge"), RANGE, metric, costs),
                lambda L, c, p: getattr(L, entry)(c, p["d_cur"], p["d_ref"], w, h, RANGE, p["d_best"], p["d_costs"], None),
                {"me_tile_rows": rows})


TILED = product(size=[(16, 16), (48, 32)], costs=[True, False], rows=[1, 0])   # frames of tiles are multiples of 16: 48 x 32 for the planar 40 x 24


@row("xSatd8x8SearchFromTilesDev", [("d_cur", 16), ("d_ref", 16), ("d_best", 8), ("d_costs", 4)], TILED)
def _(oracle, size, costs, rows):
    return _tiled_search(oracle, "xSatd8x8SearchFromTilesDev", "satd", size, costs, rows)


@row("xSad8x8SearchFromTilesDev", [("d_cur", 16), ("d_ref", 16), ("d_best", 8), ("d_costs", 4)], TILED)
def _(oracle, size, costs, rows):
    return _tiled_search(oracle, "xSad8x8SearchFromTilesDev", "sad", size, costs, rows)


def _mc_case(oracle, entry, size, luma, chroma):
    w, h = size
    y, u, v = _yuv(w, h, 270 + w)
    ref = tiles(oracle, (y, u, v), 271)
    mv = mcc._vectors(w, h, 272 + w)
    cost = (splitmix64(273, 0, len(mv)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)      # the cost field is ignored
    base = rct._tiles_mix(w, h, 274)                                                    # only the planes' masks matter
    want_y = met._mc_np(y, mv, w, h) if luma else None
    want_u, want_v, _ = mcc._mcc_np(u, v, mv, w, h) if chroma else (None, None, None)
    return Case({"d_ref": ref, "d_mv": records(mv, cost)}, {"d_pred": _recon_want(oracle, base, w, h, y=want_y, u=want_u, v=want_v)},
                lambda L, c, p: getattr(L, entry)(c, p["d_ref"], p["d_mv"], w, h, p["d_pred"], None), {})


MC_PTRS = [("d_ref", 16), ("d_mv", 8), ("d_pred", 16)]


@row("xMotionCompLumaDev", MC_PTRS, product(size=FRAMES16))
def _(oracle, size):
    return _mc_case(oracle, "xMotionCompLumaDev", size, True, False)


@row("xMotionCompChromaDev", MC_PTRS, product(size=FRAMES16))
def _(oracle, size):
    return _mc_case(oracle, "xMotionCompChromaDev", size, False, True)


@row("xMotionCompDev", MC_PTRS, product(size=FRAMES16))
def _(oracle, size):
    return _mc_case(oracle, "xMotionCompDev", size, True, True)


# ---- intra ---------------------------------------------------------------------------------------------------------------------------
def _intra_sets(n_sets, seed):
    """(refs [n, 129], the 144-byte records the device reads: garbage in the 15 reserved bytes)"""
    refs = intra_refs_np(max(n_sets, 5), seed)[:n_sets]
    padded = (splitmix64(seed + 1, 0, n_sets * 144) & np.uint64(255)).astype(np.uint8).reshape(n_sets, 144)
    padded[:, :129] = refs
    return refs, padded


def _intra_pick(n, indexed, seed):
    modes = ((np.arange(n) * 11 + seed) % 35).astype(np.uint8)
    n_sets = max(n // 2, 1) if indexed else n
    idx = (splitmix64(seed, 0, n) % np.uint64(n_sets)).astype(np.uint32) if indexed else None
    return modes, n_sets, idx


@row("xIntra32PredictDev", [("d_refs", 16), ("d_modes", 1), ("d_ref_index", 4), ("d_pred", 16)], product(n=INTRA_COUNTS, indexed=[False, True]))
def _(oracle, n, indexed):
    modes, n_sets, idx = _intra_pick(n, indexed, 280 + n)
    refs, padded = _intra_sets(n_sets, 281 + n)
    ins = {"d_refs": padded, "d_modes": modes}
    if indexed:
        ins["d_ref_index"] = idx
    return Case(ins, {"d_pred": (_b(oracle.intra32_predict(refs, modes, idx)), None)},
                lambda L, c, p: L.xIntra32PredictDev(c, p["d_refs"], p["d_modes"], p["d_ref_index"], p["d_pred"], n, None), {})


@row("xIntra32ResidualDct32Dev", [("d_refs", 16), ("d_modes", 1), ("d_ref_index", 4), ("d_src", 16), ("d_coef", 16)],
     product(n=INTRA_COUNTS, indexed=[False, True]))
def _(oracle, n, indexed):
    modes, n_sets, idx = _intra_pick(n, indexed, 290 + n)
    refs, padded = _intra_sets(n_sets, 291 + n)
    src = (splitmix64(292 + n, 0, n * 1024) & np.uint64(255)).astype(np.uint8).reshape(n, 1024)
    pred = oracle.intra32_predict(refs, modes, idx)
    want = oracle.dct32_fwd(src.astype(np.int16) - pred.astype(np.int16))
    ins = {"d_refs": padded, "d_modes": modes, "d_src": src}
    if indexed:
        ins["d_ref_index"] = idx
    return Case(ins, {"d_coef": (_b(want), None)},
                lambda L, c, p: L.xIntra32ResidualDct32Dev(c, p["d_refs"], p["d_modes"], p["d_ref_index"], p["d_src"], p["d_coef"], n, None), {})


@row("xIntra32CostsDev", [("d_refs", 16), ("d_src", 16), ("d_costs", 4), ("d_best_mode", 1)], product(n=INTRA_COUNTS, best=[True, False]))
def _(oracle, n, best):
    refs, padded = _intra_sets(n, 300 + n)
    modes = ((np.arange(n) * 11 + 3) % 35).astype(np.uint8)
    noise = ((splitmix64(301 + n, 0, n * 1024) >> np.uint64(21)) & np.uint64(15)).astype(np.int64).reshape(n, 1024) - 7
    src = np.clip(oracle.intra32_predict(refs, modes).astype(np.int64) + noise, 0, 255).astype(np.uint8)
    costs, winner = oracle.intra32_costs(refs, src)
    outs = {"d_costs": (_b(costs), None)}
    if best:
        outs["d_best_mode"] = (_b(winner), None)
    return Case({"d_refs": padded, "d_src": src}, outs,
                lambda L, c, p: L.xIntra32CostsDev(c, p["d_refs"], p["d_src"], p["d_costs"], p["d_best_mode"], n, None), {})


# ---- generators and probes ---------------------------------------------------------------------------------------------------------------
@row("xFillResidualDev", [("d_dst", 16)], product(n=[1, 7, 8, 9, 1023, 4109], wg=[64, 256]))
def _(oracle, n, wg):
    seed, first = 0x266 + n, 5 * n
    return Case({}, {"d_dst": (_b(oracle.fill_residual(n, seed, first)), None)},
                lambda L, c, p: L.xFillResidualDev(c, p["d_dst"], n, seed, first, None), {"dct32_wg_threads": wg})


@row("xHipMemCeilingDev", [("d_src", 16), ("d_dst", 16)], product(kind=[0, 1, 2, 3], nbytes=[16, 2048 + 16, 4096 * 3 + 1024 + 48]))
def _(oracle, kind, nbytes):
    src = (splitmix64(310 + nbytes, 0, nbytes // 4) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    pieces = (nbytes + 2047) // 2048
    padded = np.zeros(pieces * 512, np.uint32)
    padded[:src.size] = src
    sums = np.bitwise_xor.reduce(padded.reshape(pieces, 512), axis=1)
    assert not (sums == 0x12345678).any()                                 # the probe stores nothing
    if kind == 0:
        out = (_b(src), None)
    elif kind == 1:
        out = (_b(sums), None)
    elif kind == 2:
        pat = np.zeros(nbytes // 4, np.uint32)
        pat[0::4] = np.arange(nbytes // 16, dtype=np.uint32)
        out = (_b(pat), None)
    else:
        out = (_b(sums), np.zeros(pieces * 4, bool))                       # the whole output is a hole
    return Case({} if kind == 2 else {"d_src": src}, {"d_dst": out},
                lambda L, c, p: L.xHipMemCeilingDev(c, kind, p["d_src"], p["d_dst"], nbytes, None), {})


# ---- the table against the header: needs no GPU ------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "x266hip.h")).read()


def test_every_dev_entry_point_has_a_row():
    declared = set(re.findall(r"\b(x\w+Dev)\(", _header()))
    assert len(declared) >= 37
    assert not EXCLUDED & set(ROWS)
    assert set(ROWS) | EXCLUDED == declared, (sorted(declared - set(ROWS) - EXCLUDED), sorted((set(ROWS) | EXCLUDED) - declared))


def header_alignments(every=False):
    """{entry point: {pointer: alignment}} from the `Alignment in bytes: ...` comment in front of every ...Dev declaration (the
    placement table's calls), or with `every` in front of any declaration at all"""
    out = {}
    for items, name in re.findall(r"/\* Alignment in bytes: ([^*]+?)\. \*/\s*int (x\w+)\s*\(", _header()):
        if every or name.endswith("Dev"):
            out[name] = {k: int(v) for k, v in (i.split() for i in items.replace("\n", " ").split(","))}
    return out


def device_entry_points():
    """{entry point: [device pointer, ...]} by the form of the header's declarations, whatever the names and the layout: the context
    first, the stream last, and in between at least one device buffer -- a pointer argument d_..., or for the deblocking calls
    the pointer fields of the host-read x266_deblock_t `p`; the host-read weights `wp` are no device buffer"""
    hdr = _header()
    fields = re.findall(r"\*\s*(d_\w+)\s*;", re.search(r"typedef struct x266_deblock_t \{(.*?)\}", hdr, re.S).group(1))
    out = {}
    for name, middle in re.findall(r"^\s*int\s+(x\w+)\s*\(\s*x266hip_ctx \*ctx,([^;()]*),\s*void \*stream\s*\)\s*;", hdr, re.M):
        ptrs, other = [], []
        for type_, arg in re.findall(r"([\w ]+?)\s*\*\s*(\w+)", middle):
            if arg.startswith("d_"):
                ptrs.append(arg)
            elif "x266_deblock_t" in type_:
                ptrs += fields
            elif "x266_wp_t" not in type_:
                other.append(arg)                                         # a handle (a graph, an event)
        if ptrs:
            assert not other, (name, other)                               # a new kind of pointer: say here what it is
            out[name] = ptrs
    return out


def test_the_table_is_well_formed(oracle):
    """every variant of every row builds its inputs, extents and reference (the references are the oracle's: no GPU needed)"""
    for name, r in ROWS.items():
        assert r.variants and all(a in (1, 4, 8, 16) for a in r.ptrs.values()), name
        ids = [_vid(v) for v in r.variants]
        assert len(set(ids)) == len(ids), name
        present = set()
        for i in range(len(r.variants)):
            case = _case(oracle, name, i)
            assert case.outputs, (name, ids[i])
            present |= set(case.inputs) | set(case.outputs)
        assert present == set(r.ptrs), (name, sorted(set(r.ptrs) - present))     # every pointer is placed by some variant


# ---- running a case ------------------------------------------------------------------------------------------------------------------------
def _vid(v):
    def s(x):
        return "x".join(str(int(i)) for i in x) if isinstance(x, tuple) else str(int(x)) if isinstance(x, bool) else str(x)
    return "-".join("%s%s" % (k, s(x)) for k, x in v.items()) or "only"


@functools.lru_cache(maxsize=None)
def _case(oracle, name, index):
    """inputs and reference of one variant: computed once, shared by the placements and left unchanged"""
    r = ROWS[name]
    case = r.build(oracle, **r.variants[index])
    assert set(case.inputs) | set(case.outputs) <= set(r.ptrs) and not set(case.inputs) & set(case.outputs)
    for want, written in case.outputs.values():
        assert want.dtype == np.uint8 and (written is None or written.size == want.size)
    return case


@contextlib.contextmanager
def _options(codec, opts):
    saved = {k: codec.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            codec.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            codec.set_option(k, v)


def _launch(codec, r, case, displacement, guard_seed):
    """places every buffer, calls, waits -> (return code, arena, {output name: slot})"""
    arena, p, outs = Arena(codec), {}, {}
    for i, (name, align) in enumerate(r.ptrs.items()):
        disp, exact = displacement(i, name, align)
        if name in case.inputs:
            data = case.inputs[name]
            data, origin = data if isinstance(data, tuple) else (data, 0)
            p[name] = arena.input(name, data, exact, disp, guard_seed * 101 + i, origin=origin).ptr
        elif name in case.outputs:
            want, written = case.outputs[name]
            outs[name] = arena.output(name, want.size, exact, disp, written)
            p[name] = outs[name].ptr
        else:
            p[name] = None                                                # an optional argument this variant leaves out
    with _options(codec, case.options):
        rc = case.call(codec.L, codec.ctx, p)
        sync_or_exit(codec, rc)
    return rc, arena, outs


def _minimum(r):
    """alignment x 1, 3, 5, ... in argument order, so that the buffers' relative alignment varies too; no contract: 1"""
    return lambda i, name, align: (align * (2 * i + 1) if align > 1 else 1, align)


def _minimum_reversed(r):
    """the odd multipliers in the opposite order; no contract: 3"""
    return lambda i, name, align: (align * (2 * (len(r.ptrs) - 1 - i) + 1) if align > 1 else 3, align)


def _natural(r):
    return lambda i, name, align: (0, align)


PLACEMENTS = {"minimum": _minimum, "minimum-reversed": _minimum_reversed, "natural": _natural}


PLACED = [pytest.param(name, i, id="%s-%s" % (name, _vid(v))) for name, r in ROWS.items() for i, v in enumerate(r.variants)]


@gpu
@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("name,index", PLACED)
def test_placed(codec, oracle, name, index, placement):
    r, case = ROWS[name], _case(oracle, name, index)
    results = []
    for guard_seed in (1, 2):
        rc, arena, outs = _launch(codec, r, case, PLACEMENTS[placement](r), guard_seed)
        assert rc == 0, (rc, codec.L.xHipLastError(codec.ctx).decode())
        got = arena.check()                                               # guards, holes, inputs
        for out, (want, written) in case.outputs.items():
            sel = slice(None) if written is None else written
            bad = np.flatnonzero(got[out][sel] != want[sel])
            assert bad.size == 0, "%s (guard seed %d): %d wrong byte(s), first at written byte %d, last at %d" % (out, guard_seed, bad.size, bad[0], bad[-1])
        results.append({k: got[k] for k in case.outputs})
    for out in case.outputs:
        assert np.array_equal(results[0][out], results[1][out]), out       # the garbage around the inputs reaches no output byte


REJECTED = [pytest.param(name, ptr, id="%s-%s" % (name, ptr)) for name, r in ROWS.items() for ptr, align in r.ptrs.items() if align > 1]


@gpu
@pytest.mark.parametrize("name,ptr", REJECTED)
def test_half_alignment_is_rejected(codec, oracle, name, ptr):
    r = ROWS[name]
    index = next(i for i in range(len(r.variants)) if ptr in _case(oracle, name, i).inputs or ptr in _case(oracle, name, i).outputs)
    case = _case(oracle, name, index)
    assert codec.L.xHipSetOption(codec.ctx, b"no_such_option", 0) == EINVAL      # a known text that the call must replace
    marker = codec.L.xHipLastError(codec.ctx)
    half = r.ptrs[ptr] // 2
    rc, arena, _ = _launch(codec, r, case, lambda i, n, a: (half, half) if n == ptr else (0, a), 1)
    assert rc == EINVAL
    text = codec.L.xHipLastError(codec.ctx)
    assert text and text != marker and name.encode() in text, text
    arena.check_untouched()                                               # a rejected call launches nothing
