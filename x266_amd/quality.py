"""Frame quality (include/x266hip.h: xQualityStatsGpu, xQualityTotalsChunk, xQualityFromTotals): the numpy calls around
Codec.quality_stats_dev, built from the pieces the Codec's own numpy methods are built from.  No arithmetic lives here."""
import numpy as np

from ._lib import _P, QUALITY_CTU_DTYPE, QUALITY_SSE, QUALITY_SSIM, Codec, QualityParams, X266Error, load_library


def quality_params(**fields):
    """an x266_quality_t by field name: device addresses (absent or 0: NULL), then width, height and flags (default: both)"""
    scalars = [fields.pop("width", 0), fields.pop("height", 0), fields.pop("flags", QUALITY_SSE | QUALITY_SSIM)]
    return Codec._keyword_params(QualityParams, "quality_params", fields, scalars)


def quality_stats(codec, src_tiles, dec_tiles, w, h, flags=QUALITY_SSE | QUALITY_SSIM):
    """numpy convenience around xQualityStatsGpu: two tile arrays of a w x h frame (uint8, 512 bytes per tile) -> (records [n_ctu] of
    QUALITY_CTU_DTYPE, totals int64 [8])"""
    n_ctu = codec.ctu_count(w, h)
    d_src, d_dec, d_ctu, d_total = codec._frame(src_tiles, w, h), codec._frame(dec_tiles, w, h), codec.alloc(48 * n_ctu), codec.alloc(64)
    codec.quality_stats_dev(quality_params(d_src=d_src.ptr, d_dec=d_dec.ptr, d_ctu=d_ctu.ptr, d_total=d_total.ptr, width=w, height=h, flags=flags))
    return codec._fetch((d_ctu, QUALITY_CTU_DTYPE, (n_ctu,)), (d_total, np.int64, (8,)))


def totals_chunk():
    """xQualityTotalsChunk: CTU records the totals' workgroup of xQualityStatsGpu takes per step"""
    return int(load_library().xQualityTotalsChunk())


def from_totals(total, w, h):
    """xQualityFromTotals (host, no device): a frame's totals -> (psnr float64 [4]: Y, U, V, all; ssim float64 [3]: Y, U, V)"""
    t = np.ascontiguousarray(total, np.int64)
    psnr, ssim = np.zeros(4, np.float64), np.zeros(3, np.float64)
    if t.size != 8 or load_library().xQualityFromTotals(_P(t.ctypes.data), int(w), int(h), _P(psnr.ctypes.data), _P(ssim.ctypes.data)) != 0:
        raise X266Error("xQualityFromTotals: the sides must be positive multiples of 16 and the totals those of xQualityStatsGpu for that frame")
    return psnr, ssim
