"""ctypes view of libx266hip.so (include/x266hip.h).  No compute lives here."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_P = ctypes.c_void_p
_SZ = ctypes.c_size_t
_U64 = ctypes.c_uint64

OP_DCT32_FWD, OP_DCT32_INV, OP_SATD8X8 = 0, 1, 2
PRESET_CLOSED_FORM, PRESET_VTM_DST7, PRESET_VTM_DCT8 = 0, 1, 2


class DeblockParams(ctypes.Structure):
    """x266_deblock_t of include/x266hip.h"""
    _fields_ = [("d_class", _P), ("d_intra", _P), ("d_nnz", _P), ("d_qp", _P), ("d_mv", _P),
                ("qp", ctypes.c_int), ("beta_offset_div2", ctypes.c_int), ("tc_offset_div2", ctypes.c_int)]


class WpParams(ctypes.Structure):
    """x266_wp_t of include/x266hip.h"""
    _fields_ = [("w", (ctypes.c_int16 * 3) * 2), ("o", (ctypes.c_int16 * 3) * 2), ("log2_denom", ctypes.c_uint8 * 2)]


class LevelsParams(ctypes.Structure):
    """x266_levels_t of include/x266hip.h"""
    _fields_ = [("d_level", _P), ("d_class", _P), ("d_nnz", _P), ("d_region", _P), ("d_stream", _P), ("d_total", _P),
                ("n_regions", ctypes.c_size_t), ("cap_words", ctypes.c_uint64)]


# x266_level_region_t of include/x266hip.h
LEVEL_REGION_DTYPE = np.dtype([("cg_mask", "<u8"), ("offset", "<u8"), ("n_words", "<u4"), ("n_nz", "<u4"), ("sum_abs", "<u4"), ("max_abs", "<u4")])


class RdoqParams(ctypes.Structure):
    """x266_rdoq_t of include/x266hip.h"""
    _fields_ = [("d_coef", _P), ("d_level", _P), ("d_class", _P), ("d_qp", _P), ("d_nnz", _P), ("d_stat", _P), ("n_regions", ctypes.c_size_t),
                ("qp", ctypes.c_int), ("lambda_", ctypes.c_int)]


# x266_rdoq_region_t of include/x266hip.h
RDOQ_REGION_DTYPE = np.dtype([("dist", "<u8"), ("bits", "<u4"), ("n_nz", "<u4")])


class TDecideParams(ctypes.Structure):
    """x266_tdecide_t of include/x266hip.h"""
    _fields_ = [("d_cur", _P), ("d_pred", _P), ("d_qp", _P), ("d_cand", _P), ("d_class", _P), ("d_level", _P), ("d_nnz", _P), ("d_stat", _P),
                ("d_cost", _P), ("width", ctypes.c_int), ("height", ctypes.c_int), ("qp", ctypes.c_int), ("lambda_", ctypes.c_int),
                ("cand_luma", ctypes.c_uint16), ("cand_chroma", ctypes.c_uint16), ("class_bits", ctypes.c_uint16 * 16)]


TDECIDE_CLASSES = 0x777F        # X266_TDECIDE_CLASSES: the 13 distinct classes as a mask over class byte values


class AqParams(ctypes.Structure):
    """x266_aq_t of include/x266hip.h"""
    _fields_ = [("d_src", _P), ("d_tile", _P), ("d_total", _P), ("d_offset", _P), ("d_qp", _P), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("mode", ctypes.c_int), ("strength_q8", ctypes.c_int), ("qp", ctypes.c_int), ("chroma_qp_offset", ctypes.c_int)]


# x266_aq_tile_t of include/x266hip.h
AQ_TILE_DTYPE = np.dtype([(name, "<u4") for name in ("sum_y", "ssq_y", "sum_u", "ssq_u", "sum_v", "ssq_v", "energy", "log2_q8")])


class QualityParams(ctypes.Structure):
    """x266_quality_t of include/x266hip.h"""
    _fields_ = [("d_src", _P), ("d_dec", _P), ("d_ctu", _P), ("d_total", _P), ("width", ctypes.c_int), ("height", ctypes.c_int), ("flags", ctypes.c_int)]


# x266_quality_ctu_t of include/x266hip.h
QUALITY_CTU_DTYPE = np.dtype([("ssim", "<i8", (3,)), ("sse", "<u4", (3,)), ("win_y", "<u4"), ("win_c", "<u4"), ("reserved", "<u4")])
QUALITY_SSE, QUALITY_SSIM = 1, 2        # X266_QUALITY_SSE, X266_QUALITY_SSIM


class LaParams(ctypes.Structure):
    """x266_la_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_src", "d_low", "d_intra", "d_mode", "d_inter0", "d_inter1", "d_block", "d_total", "d_prop", "d_prop_ref0",
                                        "d_prop_ref1", "d_aq_offset", "d_offset", "d_qp")] + \
               [(name, ctypes.c_int) for name in ("width", "height", "intra_penalty", "strength_q8", "qp", "chroma_qp_offset")]


# x266_la_block_t of include/x266hip.h
LA_BLOCK_DTYPE = np.dtype([("cost", "<u4"), ("intra", "<u4"), ("mvx", "<i2"), ("mvy", "<i2"), ("kind", "u1"), ("mode", "u1"), ("reserved", "<u2")])
LA_CALLS = {"downscale": "xLaDownscaleGpu", "intra_costs": "xLaIntraCostsGpu", "frame_cost": "xLaFrameCostGpu", "propagate": "xLaPropagateGpu",
            "tree_qp": "xLaTreeQpGpu"}


class SeedParams(ctypes.Structure):
    """x266_seed_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_cur", "d_ref", "d_seed", "d_best", "d_j")] + \
               [(name, ctypes.c_int) for name in ("width", "height", "seed_scale", "centres", "range", "lambda_q4")]


class PartParams(ctypes.Structure):
    """x266_part_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_cur", "d_ref", "d_mv", "d_out", "d_level", "d_ctu", "d_nodes")] + \
               [(name, ctypes.c_int) for name in ("width", "height", "range", "lambda_q4")]


# x266_part_ctu_t of include/x266hip.h
PART_CTU_DTYPE = np.dtype([(name, "<u4") for name in ("j", "dist", "bits", "parts")])


class MotionParams(ctypes.Structure):
    """x266_motion_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_mv", "d_level", "d_ctu", "d_stream", "d_total")] + \
               [("width", ctypes.c_int), ("height", ctypes.c_int), ("cap_words", ctypes.c_uint64)]


# x266_motion_ctu_t of include/x266hip.h
MOTION_CTU_DTYPE = np.dtype([("head_mask", "<u8"), ("offset", "<u8"), ("n_words", "<u4"), ("parts", "<u4"), ("bits", "<u4"), ("max_abs", "<u4")])


class EntropyParams(ctypes.Structure):
    """x266_entropy_t of include/x266hip.h; `init` is a HOST address (or None: the default table)"""
    _fields_ = [(name, _P) for name in ("d_level", "d_class", "d_nnz", "d_region", "d_stream", "d_total", "init")] + \
               [("n_regions", ctypes.c_size_t), ("cap_words", ctypes.c_uint64)]


# x266_entropy_region_t of include/x266hip.h
ENTROPY_REGION_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("n_nz", "<u4"),
                                 ("reserved", "<u4")])
ENTROPY_CONTEXTS = 100
ENTROPY_MAX_BYTES = 6848


class EntropyMotionParams(ctypes.Structure):
    """x266_entropy_motion_t of include/x266hip.h; `init` is a HOST address (or None: the default table)"""
    _fields_ = [(name, _P) for name in ("d_ctu", "d_words", "d_coded", "d_stream", "d_total", "d_status", "init")] + \
               [("width", ctypes.c_int), ("height", ctypes.c_int), ("in_words", ctypes.c_uint64), ("cap_words", ctypes.c_uint64)]


# x266_entropy_motion_ctu_t of include/x266hip.h
ENTROPY_MOTION_CTU_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("parts", "<u4"),
                                     ("unreadable", "<u4")])
ENTROPY_MOTION_CONTEXTS = 7
ENTROPY_MOTION_MAX_BYTES = 720


class EntropySideParams(ctypes.Structure):
    """x266_entropy_side_t of include/x266hip.h; `init` is a HOST address (or None: the default table)"""
    _fields_ = [(name, _P) for name in ("d_kind", "d_mode", "d_class", "d_qp", "d_nnz", "d_coded", "d_stream", "d_total", "d_status", "init")] + \
               [("n_ctu", ctypes.c_size_t), ("cap_words", ctypes.c_uint64), ("qp", ctypes.c_int), ("chroma_qp_offset", ctypes.c_int)]


# x266_entropy_side_ctu_t of include/x266hip.h
ENTROPY_SIDE_CTU_DTYPE = np.dtype([("ctx_bins", "<u4"), ("bypass_bins", "<u4"), ("offset", "<u8"), ("n_words", "<u4"), ("n_bytes", "<u4"), ("n_intra", "<u4"),
                                   ("n_coded", "<u4")])
ENTROPY_SIDE_CONTEXTS = 16
ENTROPY_SIDE_MAX_BYTES = 80


class EntropyStatsParams(ctypes.Structure):
    """x266_entropy_stats_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_level", "d_class", "d_nnz", "d_counts", "d_part")] + [("n_regions", ctypes.c_size_t)]


class EntropySideStatsParams(ctypes.Structure):
    """x266_entropy_side_stats_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_kind", "d_mode", "d_class", "d_qp", "d_nnz", "d_counts", "d_part")] + \
               [("n_ctu", ctypes.c_size_t), ("qp", ctypes.c_int), ("chroma_qp_offset", ctypes.c_int)]


# X266_ENTROPY_STATS_REGIONS and X266_ENTROPY_SIDE_STATS_CTUS of include/x266hip.h: the regions and the CTUs of a row of d_part
ENTROPY_STATS_REGIONS = 32
ENTROPY_SIDE_STATS_CTUS = 64


class MixedParams(ctypes.Structure):
    """x266_mixed_t of include/x266hip.h"""
    _fields_ = [(name, _P) for name in ("d_cur", "d_pred", "d_qp", "d_kind_in", "d_mode_in", "d_level", "d_nnz", "d_kind", "d_mode", "d_cost", "d_recon")] + \
               [(name, ctypes.c_int) for name in ("width", "height", "qp", "rounding", "intra_penalty")]


class X266Error(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "libx266hip.so")


def build_library(force=False):
    """Compile the HIP kernels + C ABI for gfx950 in-tree (hipcc cross-compiles
    without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "--no-print-directory"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return lib_path()


_lib = None


def load_library(path=None):
    """The product library (cached), or -- path given -- another build of the same ABI, bound afresh."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    default = path is None
    path = path or lib_path()
    if not os.path.exists(path):
        raise X266Error("%s is not built (run `make -C x266_amd/csrc`); "
                        "there is no Python/CPU fallback for the kernels" % os.path.basename(path))
    L = ctypes.CDLL(path)
    L.xHipVersion.restype = ctypes.c_char_p
    L.xHipLastError.restype = ctypes.c_char_p
    L.xHipLastError.argtypes = [_P]
    L.xHipCodecInit.argtypes = [ctypes.POINTER(_P), ctypes.c_int]
    L.xHipCodecFree.argtypes = [_P]
    L.xHipCodecFree.restype = None
    L.xHipDeviceCount.restype = ctypes.c_int
    L.xHipDeviceInfo.argtypes = [_P, ctypes.c_char_p, _SZ, ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_SZ)]
    L.xHipSetOption.argtypes = [_P, ctypes.c_char_p, ctypes.c_int]
    L.xHipGetOption.argtypes = [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    L.xHipAutotuneReport.argtypes = [_P, ctypes.c_char_p, _SZ]
    for name in ("xDct32FwdBatchDev", "xDct32InvBatchDev", "xSatd8x8BatchDev"):
        getattr(L, name).argtypes = [_P, _P, _P, _SZ, _P]
    L.xDct32FwdInvBatchDev.argtypes = [_P, _P, _P, _P, _SZ, _P]
    L.xFillResidualDev.argtypes = [_P, _P, _SZ, _U64, _U64, _P]
    L.xIntra32PredictDev.argtypes = [_P, _P, _P, _P, _P, _SZ, _P]
    L.xHipStreamCreate.argtypes = [_P, ctypes.POINTER(_P)]
    L.xHipStreamDestroy.argtypes = [_P, _P]
    L.xHipGraphBegin.argtypes = [_P, _P]
    L.xHipGraphEnd.argtypes = [_P, _P, ctypes.POINTER(_P)]
    L.xHipGraphLaunch.argtypes = [_P, _P, _P]
    L.xHipGraphFree.argtypes = [_P, _P]
    L.xHipGraphFree.restype = None
    L.xIntra32CostsDev.argtypes = [_P, _P, _P, _P, _P, _SZ, _P]
    L.xIntra32ResidualDct32Dev.argtypes = [_P, _P, _P, _P, _P, _P, _SZ, _P]
    L.xTransformFwdBatchDev.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P, _SZ, _P, _P]
    L.xConvInputFmtDev.argtypes = [_P, _P, _P, _P, _P, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, _P]
    L.xConvOutput420Dev.argtypes = [_P, _P, _P, ctypes.c_ssize_t, _P, _P, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, _P]
    L.xResidualLumaDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xDct32FwdFromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSatd8x8FromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xResidualChromaDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]
    L.xDct32FwdChromaFromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]
    L.xDct32FwdCtuFromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSatd8x8ChromaFromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]
    L.xReconLumaDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xReconChromaDev.argtypes = [_P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xDct32InvToTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xDct32InvCtuToTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSadBatchDev.argtypes = [_P, ctypes.c_int, _P, _P, _P, _SZ, _P]
    L.xTransformInvBatchDev.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P, _SZ, _P, _P]
    L.xTransformTilesDev.argtypes = [_P, ctypes.c_int, _P, _P, _SZ, _P, _P, _P]
    L.xDct32PassDev.argtypes = [_P, _P, _P, _SZ, ctypes.c_int, _P]
    L.xDct32SatdFrameDev.argtypes = [_P, _P, _P, _SZ, _P, _P, _SZ, _P]
    L.xTransformSetMatrix.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P]
    L.xTransformGetMatrix.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P]
    L.xTransformUsePreset.argtypes = [_P, ctypes.c_int]
    L.xTransformPreset.argtypes = [_P]
    L.xHipMeScratchReserve.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int]
    L.xSatd8x8SearchDev.argtypes = [_P, _P, ctypes.c_ssize_t, _P, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, _P, _P, _P]
    L.xSad8x8SearchDev.argtypes = [_P, _P, ctypes.c_ssize_t, _P, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, _P, _P, _P]
    for name in ("xSatd8x8SearchFromTilesDev", "xSad8x8SearchFromTilesDev"):
        getattr(L, name).argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.xMotionCompLumaDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xMotionCompChromaDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xMotionCompDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    for name in ("xMotionCompQpelLumaGpu", "xMotionCompQpelChromaGpu", "xMotionCompQpelGpu"):
        getattr(L, name).argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSatd8x8RefineQpelFromTilesGpu.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]
    L.xMotionCompBiQpelTiles.argtypes = [_P, _P, _P, _P, _P, _P, ctypes.POINTER(WpParams), ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSatd8x8BiCostsFromTiles.argtypes = [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.POINTER(WpParams), ctypes.c_int, _P, _P, _P]
    L.xSatd8x8RefineBiQpelFromTiles.argtypes = [_P, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.POINTER(WpParams), ctypes.c_int, ctypes.c_int, _P, _P, _P]
    for name in ("xDeblockLumaGpu", "xDeblockChromaGpu", "xDeblockGpu"):
        getattr(L, name).argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeblockParams), _P, _P]
    L.xSaoStatsGpu.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xSaoDecideGpu.argtypes = [_P, _P, _SZ, ctypes.c_int, _P, _P]
    L.xSaoSearchGpu.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.xSaoApplyGpu.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.xAlfClassifyGpu.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xAlfStatsGpu.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.xAlfSumStatsGpu.argtypes = [_P, _P, _SZ, _P, _P, _P]
    L.xAlfDecideGpu.argtypes = [_P, _P, _SZ, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xAlfApplyGpu.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_int, _P, ctypes.c_int, _P, _P, _P]
    L.xLevelsPackGpu.argtypes = [_P, ctypes.POINTER(LevelsParams), _P]
    L.xLevelsUnpackGpu.argtypes = [_P, ctypes.POINTER(LevelsParams), _P]
    L.xLevelScan.argtypes = [ctypes.c_int, _P]
    L.xLevelsScanChunk.argtypes = []
    L.xLevelsScanChunk.restype = ctypes.c_uint
    L.xRdoQuantRegionsGpu.argtypes = [_P, ctypes.POINTER(RdoqParams), _P]
    L.xLevelsBitsGpu.argtypes = [_P, ctypes.POINTER(RdoqParams), _P]
    L.xTransformDecideCtuTilesGpu.argtypes = [_P, ctypes.POINTER(TDecideParams), _P]
    L.xLevelBits.argtypes = [ctypes.c_int, ctypes.c_int]
    L.xLastPosBits.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.xCgFlagBits.argtypes = [ctypes.c_int]
    L.xAqStatsGpu.argtypes = [_P, ctypes.POINTER(AqParams), _P]
    L.xAqDecideGpu.argtypes = [_P, ctypes.POINTER(AqParams), _P]
    L.xAqTotalsChunk.argtypes = []
    L.xWeightsFromTotals.argtypes = [_P, _P, ctypes.c_int, ctypes.POINTER(WpParams)]
    L.xQualityStatsGpu.argtypes = [_P, ctypes.POINTER(QualityParams), _P]
    L.xQualityTotalsChunk.argtypes = []
    L.xQualityFromTotals.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P]
    for name in LA_CALLS.values():
        getattr(L, name).argtypes = [_P, ctypes.POINTER(LaParams), _P]
    L.xSatd8x8SeededSearchGpu.argtypes = [_P, ctypes.POINTER(SeedParams), _P]
    L.xInterPartitionDecideGpu.argtypes = [_P, ctypes.POINTER(PartParams), _P]
    L.xMotionPackGpu.argtypes = [_P, ctypes.POINTER(MotionParams), _P]
    L.xMotionUnpackGpu.argtypes = [_P, ctypes.POINTER(MotionParams), _P]
    L.xMotionWalk.argtypes = [ctypes.c_int, ctypes.c_int, _SZ, ctypes.c_uint64, _P, _P]
    L.xMotionPredictor.argtypes = [ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]
    L.xMotionVectorBits.argtypes = [ctypes.c_int]
    L.xEntropyEncodeLevelsGpu.argtypes = [_P, ctypes.POINTER(EntropyParams), _P]
    L.xEntropyDecodeLevelsGpu.argtypes = [_P, ctypes.POINTER(EntropyParams), _P]
    L.xEntropyDefaultInit.argtypes = [_P]
    L.xEntropyEncodeRegion.argtypes = [_P, ctypes.c_int, _P, _P, _SZ, _P]
    L.xEntropyDecodeRegion.argtypes = [_P, _SZ, ctypes.c_int, _P, _P, _P]
    L.xEntropyEncodeMvGpu.argtypes = [_P, ctypes.POINTER(EntropyMotionParams), _P]
    L.xEntropyDecodeMvGpu.argtypes = [_P, ctypes.POINTER(EntropyMotionParams), _P]
    L.xMotionReconstructGpu.argtypes = [_P, ctypes.POINTER(MotionParams), _P]
    L.xEntropyMvDefaultInit.argtypes = [_P]
    L.xEntropyEncodeMvCtu.argtypes = [ctypes.c_int, ctypes.c_int, _SZ, ctypes.c_uint64, _P, _P, _P, _SZ, _P]
    L.xEntropyDecodeMvCtu.argtypes = [ctypes.c_int, ctypes.c_int, _SZ, _P, _SZ, _P, _P, _P, _P]
    L.xEntropyEncodeSideGpu.argtypes = [_P, ctypes.POINTER(EntropySideParams), _P]
    L.xEntropyDecodeSideGpu.argtypes = [_P, ctypes.POINTER(EntropySideParams), _P]
    L.xEntropySideDefaultInit.argtypes = [_P]
    L.xEntropyEncodeSideCtu.argtypes = [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _SZ, _P]
    L.xEntropyDecodeSideCtu.argtypes = [_P, _SZ, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P]
    L.xEntropyStatsLevelsGpu.argtypes = [_P, ctypes.POINTER(EntropyStatsParams), _P]
    L.xEntropyStatsSideGpu.argtypes = [_P, ctypes.POINTER(EntropySideStatsParams), _P]
    L.xEntropyStatsRows.argtypes = [_SZ, _SZ]
    L.xEntropyStatsRows.restype = _SZ
    L.xEntropyInitFromCounts.argtypes = [_P, _SZ, _P]
    L.xEntropyCountRegion.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P]
    L.xEntropyCountSideCtu.argtypes = [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P]
    L.xDct32CodeMixedFrameGpu.argtypes = [_P, ctypes.POINTER(MixedParams), _P]
    L.xLaTotalsChunk.argtypes = []
    L.xSceneCutFromTotals.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.xIntra32RefsFromTilesGpu.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xIntra32CodeFrameGpu.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P]
    L.xTransformCtuFromTilesDev.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.xTransformCtuToTilesDev.argtypes = [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xQuantRegionsGpu.argtypes = [_P, ctypes.c_int, _P, _P, _SZ, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.xDct32CodeCtuTilesGpu.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]
    for name in ("xDct32FwdBatch", "xDct32InvBatch", "xSatd8x8Batch"):
        getattr(L, name).argtypes = [_P, _P, _P, _SZ]
    L.xHipMalloc.argtypes = [_P, ctypes.POINTER(_P), _SZ]
    L.xHipFree.argtypes = [_P, _P]
    L.xHipHostAlloc.argtypes = [_P, ctypes.POINTER(_P), _SZ]
    L.xHipHostFree.argtypes = [_P, _P]
    L.xHipMemcpyH2D.argtypes = [_P, _P, _P, _SZ]
    L.xHipMemcpyD2H.argtypes = [_P, _P, _P, _SZ]
    L.xHipStreamSync.argtypes = [_P, _P]
    L.xHipTimeKernel.argtypes = [_P, ctypes.c_int, _P, _P, _SZ, ctypes.c_int, _P,
                                 ctypes.POINTER(ctypes.c_double)]
    L.xHipMemCeilingDev.argtypes = [_P, ctypes.c_int, _P, _P, _SZ, _P]
    L.xHipEventCreate.argtypes = [_P, ctypes.POINTER(_P)]
    L.xHipEventDestroy.argtypes = [_P, _P]
    L.xHipEventRecord.argtypes = [_P, _P, _P]
    L.xHipEventElapsedMs.argtypes = [_P, _P, _P, ctypes.POINTER(ctypes.c_double)]
    L.xDct32PackDiffRows.argtypes = [_P, ctypes.c_int, _P]
    L.xDct32PackDiffRows.restype = None
    L.xDct32PackDctWord.argtypes = [_P, ctypes.c_int]
    L.xDct32PackDctWord.restype = ctypes.c_uint64
    L.dct32_getDct.restype = ctypes.c_ulonglong
    L.satd8x8_getSatd.restype = ctypes.c_uint
    if default:
        _lib = L
    return L


def level_scan(size):
    """xLevelScan: the order in which a host coder walks a size x size block of the compact level stream, int64 [size * size]
    (entry s * 16 + i = v * size + u of scan position i of CG s).  No device."""
    pos = np.empty(max(int(size), 0) ** 2 if int(size) <= 32 else 0, np.uint16)
    if load_library().xLevelScan(int(size), _P(pos.ctypes.data if pos.size else 0)) != 0:
        raise X266Error("xLevelScan: size must be 4, 8, 16 or 32")
    return pos.astype(np.int64)


def levels_scan_chunk():
    """xLevelsScanChunk: regions the offset scan of xLevelsPackGpu takes per step"""
    return int(load_library().xLevelsScanChunk())


def level_bits(abs_level, pos_class):
    """xLevelBits: R(abs_level, pos_class) of the rate model of xRdoQuantRegionsGpu, in 1/16 bit.  No device."""
    v = int(load_library().xLevelBits(int(abs_level), int(pos_class)))
    if v < 0:
        raise X266Error("xLevelBits: abs_level must be 0..32768 and pos_class 0..2")
    return v


def last_pos_bits(u, v, log2_size):
    """xLastPosBits: Rlast(u, v) of a block of 1 << log2_size, in 1/16 bit.  No device."""
    r = int(load_library().xLastPosBits(int(u), int(v), int(log2_size)))
    if r < 0:
        raise X266Error("xLastPosBits: log2_size must be 2..5, u and v below the size")
    return r


def cg_flag_bits(coded):
    """xCgFlagBits: the cost of a coefficient group's coded flag, in 1/16 bit.  No device."""
    r = int(load_library().xCgFlagBits(int(coded)))
    if r < 0:
        raise X266Error("xCgFlagBits: coded must be 0 or 1")
    return r


def aq_totals_chunk():
    """xAqTotalsChunk: tile records the totals' workgroup of xAqStatsGpu takes per step"""
    return int(load_library().xAqTotalsChunk())


def la_totals_chunk():
    """xLaTotalsChunk: blocks the totals' workgroup of xLaFrameCostGpu takes per step"""
    return int(load_library().xLaTotalsChunk())


def scene_cut_from_totals(total, threshold_q8, frames_since_key, min_keyint, max_keyint):
    """xSceneCutFromTotals (host, no device): the totals of a P decision against the previous frame -> True for a scene cut"""
    t = np.ascontiguousarray(total, np.int64)
    rc = -1 if t.size != 8 else load_library().xSceneCutFromTotals(_P(t.ctypes.data), int(threshold_q8), int(frames_since_key), int(min_keyint), int(max_keyint))
    if rc < 0:
        raise X266Error("xSceneCutFromTotals: threshold_q8 must be 0..256, frames_since_key >= 0, 1 <= min_keyint <= max_keyint, and the totals those of "
                        "xLaFrameCostGpu")
    return bool(rc)


def pack_diff_rows(mat, first_row):
    L = load_library()
    mat = np.ascontiguousarray(mat, np.int16)
    res = np.empty(32, np.uint32)
    L.xDct32PackDiffRows(_P(mat.ctypes.data), first_row, _P(res.ctypes.data))
    return res


def pack_dct_word(dct, idx):
    L = load_library()
    dct = np.ascontiguousarray(dct, np.int16)
    return int(L.xDct32PackDctWord(_P(dct.ctypes.data), idx))


class DeviceBuffer:
    """Device allocation owned through the C ABI (xHipMalloc / xHipFree)."""

    def __init__(self, codec, nbytes):
        self.codec, self.nbytes = codec, int(nbytes)
        p = _P()
        codec._check(codec.L.xHipMalloc(codec.ctx, ctypes.byref(p), self.nbytes), "xHipMalloc")
        self.ptr = p.value or 0

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.codec._check(self.codec.L.xHipMemcpyH2D(self.codec.ctx, self.ptr, arr.ctypes.data, arr.nbytes),
                          "xHipMemcpyH2D")

    def download(self, dtype, count):
        out = np.empty(count, dtype)
        assert out.nbytes <= self.nbytes
        self.codec._check(self.codec.L.xHipMemcpyD2H(self.codec.ctx, out.ctypes.data, self.ptr, out.nbytes),
                          "xHipMemcpyD2H")
        return out

    def free(self):
        if self.ptr:
            self.codec.L.xHipFree(self.codec.ctx, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Null:
    """The buffer that stands for an absent array: NULL to the call, nothing to download."""
    ptr = 0

    def __bool__(self):
        return False


_NULL = _Null()


class Codec:
    """Context object mirroring x266hip_ctx (xHipCodecInit / xHipCodecFree)."""

    def __init__(self, device=0, library=None):
        """library: another build of the same ABI (tests: libx266hip_waits0.so) instead of the product x266_amd/libx266hip.so"""
        self.L = load_library(library)
        ctx = _P()
        rc = self.L.xHipCodecInit(ctypes.byref(ctx), int(device))
        if rc != 0 or not ctx.value:
            raise X266Error("xHipCodecInit(device=%d) failed with %d: no gfx950 device; "
                            "libx266hip has no CPU path" % (device, rc))
        self.ctx = ctx

    @classmethod
    def borrowed(cls, ctx_ptr):
        """A view of a context somebody else owns (xHipNodeCtx: a node rank's context, freed with the node)."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.ctx = _P(ctx_ptr)
        self._borrowed = True
        return self

    def close(self):
        """Frees the context.  While pinned blocks of host_alloc are still referenced the context cannot go yet (xHipHostFree needs it): the
        codec is then CLOSED FOR NEW CALLS at once -- they raise -- a ResourceWarning says so, and the context itself is freed with the
        last block (`close_deferred` is True in between)."""
        with self._lock():
            ctx = getattr(self, "ctx", None) or getattr(self, "_ctx_for_free", None)
            if not ctx:
                return
            if getattr(self, "_pinned_live", 0) > 0:
                if getattr(self, "ctx", None):
                    import warnings
                    warnings.warn("Codec.close(): %d pinned host block(s) still referenced; the codec refuses new calls now, its context is "
                                  "freed with the last block" % self._pinned_live, ResourceWarning, stacklevel=2)
                self._ctx_for_free, self.ctx = ctx, None
                return
            if not getattr(self, "_borrowed", False):
                self.L.xHipCodecFree(ctx)
            self.ctx = self._ctx_for_free = None

    @property
    def close_deferred(self):
        return bool(getattr(self, "_ctx_for_free", None))

    def _lock(self):
        lk = self.__dict__.get("_lk")
        if lk is None:
            import threading
            lk = self.__dict__.setdefault("_lk", threading.RLock())
        return lk

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            if not getattr(self, "ctx", None):
                raise X266Error("%s: the codec is closed" % what)
            raise X266Error("%s failed (%d): %s" % (what, rc, self.L.xHipLastError(self.ctx).decode()))

    # -- the pieces of the numpy convenience methods: each method is its inputs, one *_dev call, one _fetch ------------------
    def _upload(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype)
        d = self.alloc(max(a.nbytes, 16))
        d.upload(a)
        return d

    def _frame(self, tiles, w, h):
        """upload the tile array of a w x h frame (uint8, 2 bytes per luma sample)"""
        t = np.ascontiguousarray(tiles, np.uint8).ravel()
        assert t.size == w * h * 2
        return self._upload(t)

    def _out_frame(self, base, default):
        """upload what an output holds before the call: `base`, or for None `default` (zeros, or the prediction's tiles)"""
        return self._upload(np.ascontiguousarray(default if base is None else base, np.uint8).ravel())

    def _table(self, t, dtype, count=None, tail=0):
        """upload a side table of `count` elements (None: any number) and `tail` zero elements behind them; for None, _NULL"""
        if t is None:
            return _NULL
        t = np.ascontiguousarray(t, dtype).ravel()
        assert count is None or t.size == count
        return self._upload(np.concatenate([t, np.zeros(tail, t.dtype)]) if tail else t)

    def _ref_sets(self, refs):
        """upload intra reference sets [n, 129] uint8 (left | top), each padded to the 144 bytes a set takes on the device"""
        refs = np.ascontiguousarray(refs, np.uint8).reshape(-1, 129)
        padded = np.zeros((refs.shape[0], 144), np.uint8)
        padded[:, :129] = refs
        return self._upload(padded)

    @staticmethod
    def _records(mv, nb):
        """vectors [nb, 2] -> the 8-byte records (mvx, mvy, 4 bytes of cost) the motion calls read"""
        rec = np.zeros((nb, 4), np.int16)
        rec[:, :2] = np.asarray(mv, np.int16).reshape(nb, 2)
        return rec

    def _fetch(self, *outs):
        """one sync, then every (buffer, dtype, shape) downloaded: a tuple, or the array itself where there is one.  Nothing is
        downloaded for an empty shape; a NULL buffer (_NULL, an output that was not asked for) gives None"""
        self.stream_sync()
        got = tuple(np.zeros(shape, dtype) if 0 in shape else d.download(dtype, int(np.prod(shape))).reshape(shape) if d else None
                    for d, dtype, shape in outs)
        return got if len(got) > 1 else got[0]

    def _fetch_best(self, d_best, nb, d_more, shape):
        """_fetch of the search calls: their 8-byte best records and a uint32 array beside them (or _NULL)
        -> (mv [nb, 2] int16, cost [nb] uint32, that array or None)"""
        raw, more = self._fetch((d_best, np.uint8, (nb * 8,)), (d_more, np.uint32, shape))
        return raw.view(np.int16).reshape(nb, 4)[:, :2].copy(), raw.view(np.uint32).reshape(nb, 2)[:, 1].copy(), more

    @staticmethod
    def _keyword_params(struct, what, pointers, scalars):
        """a struct whose fields are pointers, given by field name (absent or 0: NULL), and then `scalars`"""
        names = [f[0] for f in struct._fields_[:-len(scalars)]]
        unknown = set(pointers) - set(names)
        if unknown:
            raise TypeError("%s: no such field: %s" % (what, sorted(unknown)))
        return struct(*([pointers.get(n) or None for n in names] + [int(s) for s in scalars]))

    # -- info / options ----------------------------------------------------
    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cu, mhz, mem = ctypes.c_int(), ctypes.c_int(), _SZ()
        self._check(self.L.xHipDeviceInfo(self.ctx, name, 256, ctypes.byref(cu), ctypes.byref(mhz),
                                          ctypes.byref(mem)), "xHipDeviceInfo")
        return {"name": name.value.decode(), "cu_count": cu.value, "clock_mhz": mhz.value,
                "hbm_bytes": mem.value}

    def set_option(self, key, value):
        self._check(self.L.xHipSetOption(self.ctx, key.encode(), int(value)), "xHipSetOption(%s)" % key)

    def get_option(self, key):
        v = ctypes.c_int()
        self._check(self.L.xHipGetOption(self.ctx, key.encode(), ctypes.byref(v)), "xHipGetOption(%s)" % key)
        return v.value

    def autotune_report(self):
        """{family: {"choice": index, "ms": [per-candidate ms]}} of the families the "autotune" option has tuned so far; under "autotune" = 2 + k
        {family: {"forced": k, "launches": count}} of the families that have launched candidate k since the option was set"""
        buf = ctypes.create_string_buffer(4096)
        self._check(self.L.xHipAutotuneReport(self.ctx, buf, len(buf)), "xHipAutotuneReport")
        out = {}
        for line in buf.value.decode().splitlines():
            w = line.split()
            if w[1] == "forced":
                out.setdefault(w[0], {}).update({"forced": int(w[2]), "launches": int(w[4])})
            else:
                out.setdefault(w[0], {}).update({"choice": int(w[2]), "ms": [float(x) for x in w[4:]]})
        return out

    # -- host-pointer batch API (numpy in, numpy out) -------------------------
    def dct32_fwd(self, x):
        x = np.ascontiguousarray(x, np.int16).reshape(-1, 1024)
        out = np.empty_like(x)
        self._check(self.L.xDct32FwdBatch(self.ctx, x.ctypes.data, out.ctypes.data, x.shape[0]), "xDct32FwdBatch")
        return out

    def dct32_inv(self, z):
        z = np.ascontiguousarray(z, np.int16).reshape(-1, 1024)
        out = np.empty_like(z)
        self._check(self.L.xDct32InvBatch(self.ctx, z.ctypes.data, out.ctypes.data, z.shape[0]), "xDct32InvBatch")
        return out

    def satd8x8(self, d):
        d = np.ascontiguousarray(d, np.int16).reshape(-1, 64)
        out = np.empty(d.shape[0], np.uint32)
        self._check(self.L.xSatd8x8Batch(self.ctx, d.ctypes.data, out.ctypes.data, d.shape[0]), "xSatd8x8Batch")
        return out

    # -- device-pointer batch API (raw pointers, e.g. torch .data_ptr()) --------
    def dct32_fwd_dev(self, d_in, d_out, n_blocks, stream=0):
        self._check(self.L.xDct32FwdBatchDev(self.ctx, d_in, d_out, n_blocks, stream), "xDct32FwdBatchDev")

    def dct32_inv_dev(self, d_in, d_out, n_blocks, stream=0):
        self._check(self.L.xDct32InvBatchDev(self.ctx, d_in, d_out, n_blocks, stream), "xDct32InvBatchDev")

    def dct32_fwd_inv_dev(self, d_in, d_coef, d_recon, n_blocks, stream=0):
        self._check(self.L.xDct32FwdInvBatchDev(self.ctx, d_in, d_coef or None, d_recon, n_blocks, stream), "xDct32FwdInvBatchDev")

    def intra32_predict_dev(self, d_refs, d_modes, d_ref_index, d_pred, n, stream=0):
        self._check(self.L.xIntra32PredictDev(self.ctx, d_refs, d_modes, d_ref_index or None, d_pred, n, stream), "xIntra32PredictDev")

    def intra32_predict(self, refs, modes, ref_index=None):
        """Host convenience: refs [n_refs,129] uint8 (left | top) -> predictions [n,1024] uint8."""
        modes = np.ascontiguousarray(modes, np.uint8)
        n = modes.shape[0]
        d_r, d_m, d_i, d_p = self._ref_sets(refs), self._upload(modes), self._table(ref_index, np.uint32), self.alloc(max(n * 1024, 16))
        self.intra32_predict_dev(d_r.ptr, d_m.ptr, d_i.ptr, d_p.ptr, n)
        return self._fetch((d_p, np.uint8, (n, 1024)))

    def intra32_residual_dct32_dev(self, d_refs, d_modes, d_ref_index, d_src, d_coef, n, stream=0):
        self._check(self.L.xIntra32ResidualDct32Dev(self.ctx, d_refs, d_modes, d_ref_index or None, d_src, d_coef, n, stream), "xIntra32ResidualDct32Dev")

    def intra32_residual_dct32(self, refs, modes, src, ref_index=None):
        """Host convenience: refs [n_refs,129] uint8, modes [n], src [n,1024] uint8 -> coefficients [n,1024] int16."""
        modes = np.ascontiguousarray(modes, np.uint8)
        n = modes.shape[0]
        d_r, d_m, d_i = self._ref_sets(refs), self._upload(modes), self._table(ref_index, np.uint32)
        d_s, d_c = self._upload(np.ascontiguousarray(src, np.uint8).reshape(-1, 1024)), self.alloc(max(n * 2048, 16))
        self.intra32_residual_dct32_dev(d_r.ptr, d_m.ptr, d_i.ptr, d_s.ptr, d_c.ptr, n)
        return self._fetch((d_c, np.int16, (n, 1024)))

    def intra32_costs_dev(self, d_refs, d_src, d_costs, d_best_mode, n, stream=0):
        self._check(self.L.xIntra32CostsDev(self.ctx, d_refs, d_src, d_costs, d_best_mode or None, n, stream), "xIntra32CostsDev")

    def intra32_costs(self, refs, src):
        """Host convenience: refs [n,129], src [n,1024] uint8 -> (costs [n,35] uint32, best_mode [n] uint8)."""
        n = np.size(refs) // 129
        d_r, d_s = self._ref_sets(refs), self._upload(np.ascontiguousarray(src, np.uint8).reshape(-1, 1024))
        d_c, d_b = self.alloc(max(n * 35 * 4, 16)), self.alloc(max(n, 16))
        self.intra32_costs_dev(d_r.ptr, d_s.ptr, d_c.ptr, d_b.ptr, n)
        return self._fetch((d_c, np.uint32, (n, 35)), (d_b, np.uint8, (n,)))

    def intra32_refs_from_tiles_dev(self, d_frame, w, h, component, d_refs, stream=0):
        self._check(self.L.xIntra32RefsFromTilesGpu(self.ctx, d_frame, w, h, int(component), d_refs, stream), "xIntra32RefsFromTilesGpu")

    def intra32_refs_from_tiles(self, tiles, w, h, component, base=None):
        """numpy convenience around xIntra32RefsFromTilesGpu: a tile array of a w x h frame (multiples of 64) -> the reference sets of
        its own samples as uint8 [n_sets, 144] (left[64] | top[65] | 15 reserved bytes): 4 per CTU for component 0, 1 for U (1) / V (2).
        `base` pre-fills the output (None: zeros)"""
        n = self.ctu_count(w, h) * (4 if component == 0 else 1)
        d_in, d_out = self._frame(tiles, w, h), self._out_frame(base, np.zeros(n * 144, np.uint8))
        self.intra32_refs_from_tiles_dev(d_in.ptr, w, h, component, d_out.ptr)
        return self._fetch((d_out, np.uint8, (n, 144)))

    def intra32_code_frame_dev(self, d_cur, w, h, d_qp, qp, rounding, d_mode_in, d_level, d_nnz, d_mode, d_recon, stream=0):
        self._check(self.L.xIntra32CodeFrameGpu(self.ctx, d_cur, w, h, d_qp or None, int(qp), int(rounding), d_mode_in or None, d_level, d_nnz or None,
                                                d_mode, d_recon, stream), "xIntra32CodeFrameGpu")

    def intra32_code_frame(self, cur_tiles, w, h, qps=None, qp=0, rounding=0, modes_in=None, base=None):
        """numpy convenience around xIntra32CodeFrameGpu: the tile array of a w x h frame (multiples of 64), optionally 6 qp bytes and 6
        mode bytes per CTU -> (levels [n_ctus, 6, 1024] int16, non-zero counts [n_ctus, 6] uint32, modes [n_ctus, 6] uint8, the
        reconstructed tile array); m_I (never written) comes from `base` (a tile array; None: zeros)"""
        n = self.ctu_count(w, h)
        dc, dr = self._frame(cur_tiles, w, h), self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        dq, dmi = self._table(qps, np.uint8, 6 * n), self._table(modes_in, np.uint8, 6 * n)
        dl, dn, dm = self.alloc(n * 12288), self.alloc(max(n * 24, 16)), self.alloc(max(n * 6, 16))
        self.intra32_code_frame_dev(dc.ptr, w, h, dq.ptr, qp, rounding, dmi.ptr, dl.ptr, dn.ptr, dm.ptr, dr.ptr)
        return self._fetch((dl, np.int16, (n, 6, 1024)), (dn, np.uint32, (n, 6)), (dm, np.uint8, (n, 6)), (dr, np.uint8, (w * h * 2,)))

    def mem_ceiling_dev(self, kind, d_src, d_dst, nbytes, stream=0):
        """kind 0 = streaming copy, 1 = read-only stream (one uint32 XOR per 2 KiB into d_dst): this box's memory ceilings"""
        self._check(self.L.xHipMemCeilingDev(self.ctx, int(kind), d_src, d_dst, nbytes, stream), "xHipMemCeilingDev")

    def satd8x8_dev(self, d_in, d_out, n_blocks, stream=0):
        self._check(self.L.xSatd8x8BatchDev(self.ctx, d_in, d_out, n_blocks, stream), "xSatd8x8BatchDev")

    def transform_fwd_dev(self, ttype, size, d_in, d_out, n_blocks, d_offsets=0, stream=0):
        self._check(self.L.xTransformFwdBatchDev(self.ctx, ttype, size, d_in, d_out, n_blocks, d_offsets or None, stream),
                    "xTransformFwdBatchDev")

    def transform_fwd(self, ttype, size, x, offsets=None, buf_samples=None):
        """numpy convenience: contiguous blocks [n, size*size], or (offsets given) a flat sample
        buffer `x` of which the blocks at `offsets` are transformed in place layout."""
        x = np.ascontiguousarray(x, np.int16)
        if offsets is None:
            n = x.size // (size * size)
            din, dout = self._upload(x), self.alloc(max(x.nbytes, 16))
            self.transform_fwd_dev(ttype, size, din.ptr, dout.ptr, n)
            return self._fetch((dout, np.int16, (n, size * size)))
        offsets = np.ascontiguousarray(offsets, np.uint32)
        din, dout, doff = self._upload(x), self._upload(np.zeros_like(x)), self._upload(offsets)
        self.transform_fwd_dev(ttype, size, din.ptr, dout.ptr, offsets.size, doff.ptr)
        return self._fetch((dout, np.int16, (x.size,)))

    def conv_input_fmt_dev(self, d_tiles, d_y, d_u, d_v, strd_y, w, h, stream=0):
        self._check(self.L.xConvInputFmtDev(self.ctx, d_tiles, d_y, d_u, d_v, strd_y, w, h, stream), "xConvInputFmtDev")

    def conv_output_420_dev(self, d_tiles, d_y, strd_y, d_u, d_v, strd_c, w, h, stream=0):
        self._check(self.L.xConvOutput420Dev(self.ctx, d_tiles, d_y, strd_y, d_u, d_v, strd_c, w, h, stream), "xConvOutput420Dev")

    def residual_luma_dev(self, d_cur, d_pred, w, h, edge, d_res, stream=0):
        self._check(self.L.xResidualLumaDev(self.ctx, d_cur, d_pred, w, h, edge, d_res, stream), "xResidualLumaDev")

    def dct32_fwd_from_tiles_dev(self, d_cur, d_pred, w, h, d_coef, stream=0):
        self._check(self.L.xDct32FwdFromTilesDev(self.ctx, d_cur, d_pred, w, h, d_coef, stream), "xDct32FwdFromTilesDev")

    def satd8x8_from_tiles_dev(self, d_cur, d_pred, w, h, d_out, stream=0):
        self._check(self.L.xSatd8x8FromTilesDev(self.ctx, d_cur, d_pred, w, h, d_out, stream), "xSatd8x8FromTilesDev")

    def residual_chroma_dev(self, d_cur, d_pred, w, h, edge, d_res_u, d_res_v, block_pitch=1, stream=0):
        self._check(self.L.xResidualChromaDev(self.ctx, d_cur, d_pred, w, h, edge, d_res_u, d_res_v, block_pitch, stream), "xResidualChromaDev")

    def dct32_fwd_chroma_from_tiles_dev(self, d_cur, d_pred, w, h, d_coef_u, d_coef_v, block_pitch=1, stream=0):
        self._check(self.L.xDct32FwdChromaFromTilesDev(self.ctx, d_cur, d_pred, w, h, d_coef_u, d_coef_v, block_pitch, stream),
                    "xDct32FwdChromaFromTilesDev")

    def dct32_fwd_ctu_from_tiles_dev(self, d_cur, d_pred, w, h, d_coef, stream=0):
        self._check(self.L.xDct32FwdCtuFromTilesDev(self.ctx, d_cur, d_pred, w, h, d_coef, stream), "xDct32FwdCtuFromTilesDev")

    def satd8x8_chroma_from_tiles_dev(self, d_cur, d_pred, w, h, d_out_u, d_out_v, pitch=1, stream=0):
        self._check(self.L.xSatd8x8ChromaFromTilesDev(self.ctx, d_cur, d_pred, w, h, d_out_u, d_out_v, pitch, stream),
                    "xSatd8x8ChromaFromTilesDev")

    def recon_luma_dev(self, d_pred, d_res, w, h, edge, d_recon, stream=0):
        self._check(self.L.xReconLumaDev(self.ctx, d_pred, d_res, w, h, edge, d_recon, stream), "xReconLumaDev")

    def recon_chroma_dev(self, d_pred, d_res_u, d_res_v, w, h, edge, d_recon, block_pitch=1, stream=0):
        self._check(self.L.xReconChromaDev(self.ctx, d_pred, d_res_u, d_res_v, block_pitch, w, h, edge, d_recon, stream), "xReconChromaDev")

    def dct32_inv_to_tiles_dev(self, d_coef, d_pred, w, h, d_recon, stream=0):
        self._check(self.L.xDct32InvToTilesDev(self.ctx, d_coef, d_pred, w, h, d_recon, stream), "xDct32InvToTilesDev")

    def dct32_inv_ctu_to_tiles_dev(self, d_coef, d_pred, w, h, d_recon, stream=0):
        self._check(self.L.xDct32InvCtuToTilesDev(self.ctx, d_coef, d_pred, w, h, d_recon, stream), "xDct32InvCtuToTilesDev")

    def sad_dev(self, edge, d_a, d_b, d_out, n_blocks, stream=0):
        self._check(self.L.xSadBatchDev(self.ctx, edge, d_a, d_b, d_out, n_blocks, stream), "xSadBatchDev")

    def sad(self, edge, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, edge * edge)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, edge * edge)
        n = a.shape[0]
        da, db, do = self._upload(a), self._upload(b), self.alloc(max(4 * n, 16))
        self.sad_dev(edge, da.ptr, db.ptr, do.ptr, n)
        return self._fetch((do, np.uint32, (n,)))

    def transform_tiles_dev(self, inverse, d_in, d_out, n_tiles, d_tile_offsets, d_tile_class, stream=0):
        self._check(self.L.xTransformTilesDev(self.ctx, int(inverse), d_in, d_out, n_tiles, d_tile_offsets or None, d_tile_class, stream),
                    "xTransformTilesDev")

    def frame_lanes_dev(self, d_dct_in, d_dct_out, n_dct, d_diff, d_satd_out, n_satd, stream=0):
        self._check(self.L.xDct32SatdFrameDev(self.ctx, d_dct_in, d_dct_out, n_dct, d_diff, d_satd_out, n_satd, stream), "xDct32SatdFrameDev")

    def dct32_pass(self, x, shift):
        """numpy convenience around xDct32PassDev: [n, 1024] int16 -> the 1-D pass of every block, stored transposed."""
        x = np.ascontiguousarray(x, np.int16).reshape(-1, 1024)
        din, dout = self._upload(x), self.alloc(max(x.nbytes, 16))
        self._check(self.L.xDct32PassDev(self.ctx, din.ptr, dout.ptr, x.shape[0], int(shift), None), "xDct32PassDev")
        return self._fetch((dout, np.int16, x.shape))

    def set_transform_matrix(self, slot, size, m=None):
        """Install an N x N int8 matrix (row k = basis function) in 1-D transform slot 0 / 1; None restores the built-in."""
        if m is None:
            self._check(self.L.xTransformSetMatrix(self.ctx, slot, size, None), "xTransformSetMatrix")
            return
        m = np.ascontiguousarray(m, np.int8)
        assert m.shape == (size, size)
        self._check(self.L.xTransformSetMatrix(self.ctx, slot, size, m.ctypes.data), "xTransformSetMatrix")

    def use_transform_preset(self, preset):
        """0 closed-form DST-VII (built-in), 1 H.266 DST-VII as recalled from VTM, 2 DCT-VIII derived from it -- slot 1, all sizes"""
        self._check(self.L.xTransformUsePreset(self.ctx, int(preset)), "xTransformUsePreset")

    def transform_preset(self):
        return self.L.xTransformPreset(self.ctx)

    def get_transform_matrix(self, slot, size):
        m = np.empty((size, size), np.int8)
        self._check(self.L.xTransformGetMatrix(self.ctx, slot, size, m.ctypes.data), "xTransformGetMatrix")
        return m

    def transform_inv_dev(self, ttype, size, d_in, d_out, n_blocks, d_offsets=0, stream=0):
        self._check(self.L.xTransformInvBatchDev(self.ctx, ttype, size, d_in, d_out, n_blocks, d_offsets or None, stream), "xTransformInvBatchDev")

    def transform_inv(self, ttype, size, x):
        x = np.ascontiguousarray(x, np.int16)
        n = x.size // (size * size)
        din, dout = self._upload(x), self.alloc(max(x.nbytes, 16))
        self.transform_inv_dev(ttype, size, din.ptr, dout.ptr, n)
        return self._fetch((dout, np.int16, (n, size * size)))

    def satd_search_dev(self, d_cur, cur_stride, d_ref_origin, ref_stride, width, height, rng, d_best, d_costs=0,
                        stream=0):
        self._check(self.L.xSatd8x8SearchDev(self.ctx, d_cur, cur_stride, d_ref_origin, ref_stride, width, height,
                                             rng, d_best, d_costs or None, stream), "xSatd8x8SearchDev")

    def sad_search_dev(self, d_cur, cur_stride, d_ref_origin, ref_stride, width, height, rng, d_best, d_costs=0,
                       stream=0):
        self._check(self.L.xSad8x8SearchDev(self.ctx, d_cur, cur_stride, d_ref_origin, ref_stride, width, height,
                                            rng, d_best, d_costs or None, stream), "xSad8x8SearchDev")

    def satd_search(self, cur, ref_padded, pad, rng, want_costs=False, metric="satd"):
        """numpy convenience around xSatd8x8SearchDev / xSad8x8SearchDev: cur [H,W] uint8, ref_padded [H+2*pad, W+2*pad]."""
        cur = np.ascontiguousarray(cur, np.uint8)
        refp = np.ascontiguousarray(ref_padded, np.uint8)
        h, w = cur.shape
        nb, ncand = (h // 8) * (w // 8), (2 * rng + 1) ** 2
        dc, dr, db = self._upload(cur), self._upload(refp), self.alloc(nb * 8)
        dcost = self.alloc(nb * ncand * 4) if want_costs else _NULL
        fn = self.satd_search_dev if metric == "satd" else self.sad_search_dev
        fn(dc.ptr, cur.strides[0], dr.ptr + pad * refp.strides[0] + pad, refp.strides[0], w, h, rng, db.ptr, dcost.ptr)
        return self._fetch_best(db, nb, dcost, (nb, ncand))

    def satd_search_from_tiles_dev(self, d_cur, d_ref, width, height, rng, d_best, d_costs=0, stream=0):
        self._check(self.L.xSatd8x8SearchFromTilesDev(self.ctx, d_cur, d_ref, width, height, rng, d_best, d_costs or None, stream),
                    "xSatd8x8SearchFromTilesDev")

    def sad_search_from_tiles_dev(self, d_cur, d_ref, width, height, rng, d_best, d_costs=0, stream=0):
        self._check(self.L.xSad8x8SearchFromTilesDev(self.ctx, d_cur, d_ref, width, height, rng, d_best, d_costs or None, stream),
                    "xSad8x8SearchFromTilesDev")

    def motion_comp_luma_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompLumaDev(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompLumaDev")

    def motion_comp_chroma_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompChromaDev(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompChromaDev")

    def motion_comp_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompDev(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompDev")

    def search_tiles(self, cur_tiles, ref_tiles, w, h, rng, want_costs=False, metric="satd"):
        """numpy convenience around xSatd8x8SearchFromTilesDev / xSad8x8SearchFromTilesDev: two tile arrays of a w x h frame
        (uint8, 512 bytes per tile) -> (mv [nb, 2] int16, cost [nb] uint32, costs [nb, (2R+1)^2] or None), as satd_search."""
        nb, ncand = (h // 8) * (w // 8), (2 * rng + 1) ** 2
        dc, dr, db = self._frame(cur_tiles, w, h), self._frame(ref_tiles, w, h), self.alloc(nb * 8)
        dcost = self.alloc(nb * ncand * 4) if want_costs else _NULL
        fn = self.satd_search_from_tiles_dev if metric == "satd" else self.sad_search_from_tiles_dev
        fn(dc.ptr, dr.ptr, w, h, rng, db.ptr, dcost.ptr)
        return self._fetch_best(db, nb, dcost, (nb, ncand))

    def _motion_comp(self, fn, ref_tiles, mv, w, h, base):
        dr, dm = self._frame(ref_tiles, w, h), self._upload(self._records(mv, (h // 8) * (w // 8)))
        dp = self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        fn(dr.ptr, dm.ptr, w, h, dp.ptr)
        return self._fetch((dp, np.uint8, (w * h * 2,)))

    def motion_comp_luma(self, ref_tiles, mv, w, h, base=None):
        """numpy convenience around xMotionCompLumaDev: ref tile array, mv [nb, 2] int16 (mvx, mvy per 8x8 block, raster order)
        -> the predicted tile array; m_C / m_I come from `base` (a tile array; None: zeros), as the call leaves them."""
        return self._motion_comp(self.motion_comp_luma_dev, ref_tiles, mv, w, h, base)

    def motion_comp(self, ref_tiles, mv, w, h, base=None, planes="both"):
        """numpy convenience around xMotionCompDev (planes="both") / xMotionCompChromaDev (planes="chroma"): as motion_comp_luma;
        what the call does not write (m_I, and m_Y for "chroma") comes from `base`."""
        return self._motion_comp({"both": self.motion_comp_dev, "chroma": self.motion_comp_chroma_dev}[planes], ref_tiles, mv, w, h, base)

    def motion_comp_qpel_luma_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompQpelLumaGpu(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompQpelLumaGpu")

    def motion_comp_qpel_chroma_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompQpelChromaGpu(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompQpelChromaGpu")

    def motion_comp_qpel_dev(self, d_ref, d_mv, width, height, d_pred, stream=0):
        self._check(self.L.xMotionCompQpelGpu(self.ctx, d_ref, d_mv, width, height, d_pred, stream), "xMotionCompQpelGpu")

    def satd_refine_qpel_from_tiles_dev(self, d_cur, d_ref, width, height, d_int, d_best, d_costs=0, stream=0):
        self._check(self.L.xSatd8x8RefineQpelFromTilesGpu(self.ctx, d_cur, d_ref, width, height, d_int, d_best, d_costs or None, stream),
                    "xSatd8x8RefineQpelFromTilesGpu")

    def motion_comp_qpel(self, ref_tiles, mv, w, h, base=None, planes="both"):
        """numpy convenience around xMotionCompQpelGpu (planes="both") / ...LumaGpu ("luma") / ...ChromaGpu ("chroma"): ref tile
        array, mv [nb, 2] int16 in quarter luma samples per 8x8 block -> the predicted tile array; what the call does not write
        comes from `base` (a tile array; None: zeros)."""
        fn = {"both": self.motion_comp_qpel_dev, "luma": self.motion_comp_qpel_luma_dev, "chroma": self.motion_comp_qpel_chroma_dev}[planes]
        return self._motion_comp(fn, ref_tiles, mv, w, h, base)

    def refine_qpel_tiles(self, cur_tiles, ref_tiles, w, h, mv_int, want_costs=False):
        """numpy convenience around xSatd8x8RefineQpelFromTilesGpu: two tile arrays and integer vectors [nb, 2] int16 ->
        (mv [nb, 2] int16 in quarter samples, cost [nb] uint32, costs [nb, 49] or None)."""
        nb = (h // 8) * (w // 8)
        dc, dr, di, db = self._frame(cur_tiles, w, h), self._frame(ref_tiles, w, h), self._upload(self._records(mv_int, nb)), self.alloc(nb * 8)
        dcost = self.alloc(nb * 49 * 4) if want_costs else _NULL
        self.satd_refine_qpel_from_tiles_dev(dc.ptr, dr.ptr, w, h, di.ptr, db.ptr, dcost.ptr)
        return self._fetch_best(db, nb, dcost, (nb, 49))

    @staticmethod
    def wp_params(w=((1, 1, 1), (1, 1, 1)), o=((0, 0, 0), (0, 0, 0)), log2_denom=(0, 0)):
        """an x266_wp_t: w and o indexed [list][Y, U, V], log2_denom [luma, chroma]; the defaults are the default weights"""
        p = WpParams()
        for l in range(2):
            for c in range(3):
                p.w[l][c], p.o[l][c] = int(w[l][c]), int(o[l][c])
        p.log2_denom[0], p.log2_denom[1] = int(log2_denom[0]), int(log2_denom[1])
        return p

    def motion_comp_bi_qpel_dev(self, d_ref0, d_ref1, d_mv0, d_mv1, width, height, d_pred, d_dir=0, wp=None, planes=3, stream=0):
        self._check(self.L.xMotionCompBiQpelTiles(self.ctx, d_ref0, d_ref1, d_mv0, d_mv1, d_dir or None, ctypes.byref(wp) if wp is not None else None,
                                                  planes, width, height, d_pred, stream), "xMotionCompBiQpelTiles")

    def satd8x8_bi_costs_dev(self, d_cur, d_ref0, d_ref1, width, height, d_mv0, d_mv1, d_costs=0, d_dir=0, wp=None, bi_penalty=0, stream=0):
        self._check(self.L.xSatd8x8BiCostsFromTiles(self.ctx, d_cur, d_ref0, d_ref1, width, height, d_mv0, d_mv1, ctypes.byref(wp) if wp is not None else None,
                                                    int(bi_penalty), d_costs or None, d_dir or None, stream), "xSatd8x8BiCostsFromTiles")

    def satd8x8_refine_bi_qpel_dev(self, d_cur, d_ref_fix, d_mv_fix, d_ref, d_int, lst, width, height, d_best, d_costs=0, wp=None, stream=0):
        self._check(self.L.xSatd8x8RefineBiQpelFromTiles(self.ctx, d_cur, d_ref_fix, d_mv_fix, d_ref, d_int, int(lst),
                                                         ctypes.byref(wp) if wp is not None else None, width, height, d_best, d_costs or None, stream),
                    "xSatd8x8RefineBiQpelFromTiles")

    def motion_comp_bi_qpel(self, ref0_tiles, ref1_tiles, mv0, mv1, w, h, direction=None, wp=None, planes=3, base=None):
        """numpy convenience around xMotionCompBiQpelTiles: two reference tile arrays (ref1_tiles None: the same buffer as list 0), mv0 /
        mv1 [nb, 2] int16 in quarter luma samples, direction uint8 [nb] or None (every block 3), wp from wp_params() or None ->
        the predicted tile array; what the call does not write comes from `base` (a tile array; None: zeros)."""
        nb = (h // 8) * (w // 8)
        d0 = self._frame(ref0_tiles, w, h)
        d1 = d0 if ref1_tiles is None else self._frame(ref1_tiles, w, h)
        dm0, dm1, dd = self._upload(self._records(mv0, nb)), self._upload(self._records(mv1, nb)), self._table(direction, np.uint8, nb)
        dp = self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        self.motion_comp_bi_qpel_dev(d0.ptr, d1.ptr, dm0.ptr, dm1.ptr, w, h, dp.ptr, dd.ptr, wp, planes)
        return self._fetch((dp, np.uint8, (w * h * 2,)))

    def satd8x8_bi_costs(self, cur_tiles, ref0_tiles, ref1_tiles, w, h, mv0, mv1, wp=None, bi_penalty=0):
        """numpy convenience around xSatd8x8BiCostsFromTiles -> (costs [nb, 3] uint32, direction [nb] uint8)"""
        nb = (h // 8) * (w // 8)
        dc, d0, d1 = (self._frame(t, w, h) for t in (cur_tiles, ref0_tiles, ref1_tiles))
        dm0, dm1 = self._upload(self._records(mv0, nb)), self._upload(self._records(mv1, nb))
        dk, dd = self.alloc(nb * 12), self.alloc(max(nb, 16))
        self.satd8x8_bi_costs_dev(dc.ptr, d0.ptr, d1.ptr, w, h, dm0.ptr, dm1.ptr, dk.ptr, dd.ptr, wp, bi_penalty)
        return self._fetch((dk, np.uint32, (nb, 3)), (dd, np.uint8, (nb,)))

    def satd8x8_refine_bi_qpel(self, cur_tiles, ref_fix_tiles, mv_fix, ref_tiles, mv_int, lst, w, h, wp=None, want_costs=False):
        """numpy convenience around xSatd8x8RefineBiQpelFromTiles: mv_fix [nb, 2] int16 in quarter samples, mv_int [nb, 2] integer vectors
        of the list `lst` being refined -> (mv [nb, 2] int16 in quarter samples, cost [nb] uint32, costs [nb, 49] or None)."""
        nb = (h // 8) * (w // 8)
        dc, df, dr = (self._frame(t, w, h) for t in (cur_tiles, ref_fix_tiles, ref_tiles))
        dmf, di, db = self._upload(self._records(mv_fix, nb)), self._upload(self._records(mv_int, nb)), self.alloc(nb * 8)
        dcost = self.alloc(nb * 49 * 4) if want_costs else _NULL
        self.satd8x8_refine_bi_qpel_dev(dc.ptr, df.ptr, dmf.ptr, dr.ptr, di.ptr, lst, w, h, db.ptr, dcost.ptr, wp)
        return self._fetch_best(db, nb, dcost, (nb, 49))

    @staticmethod
    def deblock_params(d_class=0, d_intra=0, d_nnz=0, d_qp=0, d_mv=0, qp=0, beta_offset_div2=0, tc_offset_div2=0):
        """an x266_deblock_t from device addresses (0: NULL, the documented default of that array)"""
        return DeblockParams(d_class or None, d_intra or None, d_nnz or None, d_qp or None, d_mv or None, qp, beta_offset_div2, tc_offset_div2)

    def deblock_luma_dev(self, d_in, width, height, params, d_out, stream=0):
        self._check(self.L.xDeblockLumaGpu(self.ctx, d_in, width, height, ctypes.byref(params), d_out, stream), "xDeblockLumaGpu")

    def deblock_chroma_dev(self, d_in, width, height, params, d_out, stream=0):
        self._check(self.L.xDeblockChromaGpu(self.ctx, d_in, width, height, ctypes.byref(params), d_out, stream), "xDeblockChromaGpu")

    def deblock_dev(self, d_in, width, height, params, d_out, stream=0):
        self._check(self.L.xDeblockGpu(self.ctx, d_in, width, height, ctypes.byref(params), d_out, stream), "xDeblockGpu")

    def deblock(self, tiles, w, h, planes="both", in_place=False, base=None, cls=None, intra=None, nnz=None, qps=None, mv=None,
                qp=0, beta_offset_div2=0, tc_offset_div2=0):
        """numpy convenience around xDeblockGpu (planes="both") / xDeblockLumaGpu ("luma") / xDeblockChromaGpu ("chroma"): a tile
        array and the side arrays of x266_deblock_t (cls, intra, qps: uint8 [6 n_ctu]; nnz: uint32 [6 n_ctu]; mv: int16 [nb, 2] in
        quarter samples; None: NULL) -> the deblocked tile array.  in_place: d_out == d_in; otherwise what the call does not write
        comes from `base` (a tile array; None: zeros)."""
        fn = {"both": self.deblock_dev, "luma": self.deblock_luma_dev, "chroma": self.deblock_chroma_dev}[planes]
        rec = None if mv is None else self._records(mv, (h // 8) * (w // 8))
        side = [self._table(t, dtype) for t, dtype in ((cls, np.uint8), (intra, np.uint8), (nnz, np.uint32), (qps, np.uint8), (rec, np.int16))]
        params = self.deblock_params(*[d.ptr for d in side], qp, beta_offset_div2, tc_offset_div2)
        d_in = self._frame(tiles, w, h)
        d_out = d_in if in_place else self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        fn(d_in.ptr, w, h, params, d_out.ptr)
        return self._fetch((d_out, np.uint8, (w * h * 2,)))

    def sao_stats_dev(self, d_org, d_dec, width, height, d_stats, stream=0):
        self._check(self.L.xSaoStatsGpu(self.ctx, d_org, d_dec, width, height, d_stats, stream), "xSaoStatsGpu")

    def sao_decide_dev(self, d_stats, n_ctu, lambda_q4, d_param, stream=0):
        self._check(self.L.xSaoDecideGpu(self.ctx, d_stats, n_ctu, int(lambda_q4), d_param, stream), "xSaoDecideGpu")

    def sao_search_dev(self, d_org, d_dec, width, height, lambda_q4, d_param, d_stats=0, stream=0):
        self._check(self.L.xSaoSearchGpu(self.ctx, d_org, d_dec, width, height, int(lambda_q4), d_param, d_stats or None, stream), "xSaoSearchGpu")

    def sao_apply_dev(self, d_in, width, height, d_param, d_out, stream=0):
        self._check(self.L.xSaoApplyGpu(self.ctx, d_in, width, height, d_param, d_out, stream), "xSaoApplyGpu")

    def sao_stats(self, org_tiles, dec_tiles, w, h):
        """numpy convenience around xSaoStatsGpu: the source and the decoded tile array -> int32 [n_ctu, 3, 48, 2] (count, sum)"""
        n = self.ctu_count(w, h)
        d_org, d_dec, d_stats = self._frame(org_tiles, w, h), self._frame(dec_tiles, w, h), self.alloc(n * 1152)
        self.sao_stats_dev(d_org.ptr, d_dec.ptr, w, h, d_stats.ptr)
        return self._fetch((d_stats, np.int32, (n, 3, 48, 2)))

    def sao_decide(self, stats, lambda_q4):
        """numpy convenience around xSaoDecideGpu: int32 [n_ctu, 3, 48, 2] -> the x266_sao_t records as uint8 [n_ctu, 3, 8]"""
        st = np.ascontiguousarray(stats, np.int32).reshape(-1, 3, 48, 2)
        n = st.shape[0]
        d_stats, d_param = self._upload(st), self.alloc(max(n * 24, 16))
        self.sao_decide_dev(d_stats.ptr, n, lambda_q4, d_param.ptr)
        return self._fetch((d_param, np.uint8, (n, 3, 8)))

    def sao_search(self, org_tiles, dec_tiles, w, h, lambda_q4, want_stats=False):
        """numpy convenience around xSaoSearchGpu: two tile arrays -> (records uint8 [n_ctu, 3, 8], statistics or None)"""
        n = self.ctu_count(w, h)
        d_org, d_dec, d_param = self._frame(org_tiles, w, h), self._frame(dec_tiles, w, h), self.alloc(n * 24)
        d_stats = self.alloc(n * 1152) if want_stats else _NULL
        self.sao_search_dev(d_org.ptr, d_dec.ptr, w, h, lambda_q4, d_param.ptr, d_stats.ptr)
        return self._fetch((d_param, np.uint8, (n, 3, 8)), (d_stats, np.int32, (n, 3, 48, 2)))

    def sao_apply(self, tiles, w, h, params, base=None):
        """numpy convenience around xSaoApplyGpu: a tile array and the records (uint8 [n_ctu, 3, 8]) -> the filtered tile array; m_I,
        which the call does not write, comes from `base` (a tile array; None: zeros)"""
        d_in, d_par = self._frame(tiles, w, h), self._table(params, np.uint8, self.ctu_count(w, h) * 24)
        d_out = self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        self.sao_apply_dev(d_in.ptr, w, h, d_par.ptr, d_out.ptr)
        return self._fetch((d_out, np.uint8, (w * h * 2,)))

    # ---- adaptive loop filter: 2358 int32 of statistics per CTU, one class byte per 4x4 luma block, 3 control bytes per CTU
    ALF_CTU_WORDS = 2358

    def alf_classify_dev(self, d_dec, width, height, d_class, stream=0):
        self._check(self.L.xAlfClassifyGpu(self.ctx, d_dec, width, height, d_class, stream), "xAlfClassifyGpu")

    def alf_stats_dev(self, d_org, d_dec, width, height, d_class, d_stats, stream=0):
        self._check(self.L.xAlfStatsGpu(self.ctx, d_org, d_dec, width, height, d_class or None, d_stats, stream), "xAlfStatsGpu")

    def alf_sum_stats_dev(self, d_stats, n_ctu, d_mask, d_total, stream=0):
        self._check(self.L.xAlfSumStatsGpu(self.ctx, d_stats, n_ctu, d_mask or None, d_total, stream), "xAlfSumStatsGpu")

    def alf_decide_dev(self, d_stats, n_ctu, d_luma, n_luma, d_chroma, n_chroma, lambda_q4, d_ctrl, stream=0):
        self._check(self.L.xAlfDecideGpu(self.ctx, d_stats, n_ctu, d_luma or None, int(n_luma), d_chroma or None, int(n_chroma), int(lambda_q4), d_ctrl,
                                         stream), "xAlfDecideGpu")

    def alf_apply_dev(self, d_in, width, height, d_class, d_luma, n_luma, d_chroma, n_chroma, d_ctrl, d_out, stream=0):
        self._check(self.L.xAlfApplyGpu(self.ctx, d_in, width, height, d_class or None, d_luma or None, int(n_luma), d_chroma or None, int(n_chroma),
                                        d_ctrl, d_out, stream), "xAlfApplyGpu")

    @staticmethod
    def alf_pack_filters(luma_coef=None, luma_clip=None, chroma_coef=None, chroma_clip=None):
        """filter sets from numpy arrays -> (x266_alf_luma_t array as uint8 [n_luma, 600], x266_alf_chroma_t array as uint8 [n_chroma, 16]).
        luma_coef: int [n_luma, 25, 12] in -128..127, luma_clip: the clip indices 0..3 of the same shape (None: 0); chroma_coef:
        int [n_chroma, 6], chroma_clip likewise; a missing kind gives an array of no sets."""
        def pack(coef, clip, shape, size):
            if coef is None:
                return np.zeros((0, size), np.uint8)
            c = np.asarray(coef, np.int64).reshape((-1,) + shape)
            k = np.zeros_like(c) if clip is None else np.asarray(clip, np.int64).reshape(c.shape)
            assert c.shape[0] <= 8 and c.min() >= -128 and c.max() <= 127 and k.min() >= 0 and k.max() <= 255
            n, taps = c.shape[0], int(np.prod(shape))
            out = np.zeros((n, size), np.uint8)
            out[:, :taps] = c.astype(np.int8).reshape(n, taps).view(np.uint8)
            out[:, taps:2 * taps] = k.astype(np.uint8).reshape(n, taps)
            return out
        return pack(luma_coef, luma_clip, (25, 12), 600), pack(chroma_coef, chroma_clip, (6,), 16)

    def _alf_sets(self, luma, chroma):
        luma = np.zeros((0, 600), np.uint8) if luma is None else np.ascontiguousarray(luma, np.uint8).reshape(-1, 600)
        chroma = np.zeros((0, 16), np.uint8) if chroma is None else np.ascontiguousarray(chroma, np.uint8).reshape(-1, 16)
        d_luma, d_chroma = (self._upload(s if s.size else np.zeros(16, np.uint8)) for s in (luma, chroma))
        return d_luma, luma.shape[0], d_chroma, chroma.shape[0]

    def alf_classify(self, tiles, w, h):
        """numpy convenience around xAlfClassifyGpu: a tile array -> the class bytes uint8 [h / 4, w / 4] (class | tr << 5)"""
        d_in, d_cls = self._frame(tiles, w, h), self.alloc(max((w // 4) * (h // 4), 16))
        self.alf_classify_dev(d_in.ptr, w, h, d_cls.ptr)
        return self._fetch((d_cls, np.uint8, (h // 4, w // 4)))

    def alf_stats(self, org_tiles, dec_tiles, w, h, classes=None):
        """numpy convenience around xAlfStatsGpu: the source and the decoded tile array (and a class map, None: classified inside)
        -> int32 [n_ctu, 2358]"""
        n = self.ctu_count(w, h)
        d_org, d_dec, d_cls = self._frame(org_tiles, w, h), self._frame(dec_tiles, w, h), self._table(classes, np.uint8)
        d_stats = self.alloc(n * self.ALF_CTU_WORDS * 4)
        self.alf_stats_dev(d_org.ptr, d_dec.ptr, w, h, d_cls.ptr, d_stats.ptr)
        return self._fetch((d_stats, np.int32, (n, self.ALF_CTU_WORDS)))

    def alf_sum_stats(self, stats, mask=None):
        """numpy convenience around xAlfSumStatsGpu: int32 [n_ctu, 2358] (and a byte per CTU, None: all) -> int64 [2358]"""
        st = np.ascontiguousarray(stats, np.int32).reshape(-1, self.ALF_CTU_WORDS)
        n = st.shape[0]
        d_stats, d_total, d_mask = self._upload(st), self._upload(np.zeros(self.ALF_CTU_WORDS, np.int64)), self._table(mask, np.uint8, n)
        self.alf_sum_stats_dev(d_stats.ptr, n, d_mask.ptr, d_total.ptr)
        return self._fetch((d_total, np.int64, (self.ALF_CTU_WORDS,)))

    def alf_decide(self, stats, luma, chroma, lambda_q4):
        """numpy convenience around xAlfDecideGpu: int32 [n_ctu, 2358] and the packed sets of alf_pack_filters -> d_ctrl uint8 [n_ctu, 3]"""
        st = np.ascontiguousarray(stats, np.int32).reshape(-1, self.ALF_CTU_WORDS)
        n = st.shape[0]
        d_stats, d_ctrl = self._upload(st), self.alloc(max(3 * n, 16))
        d_luma, n_luma, d_chroma, n_chroma = self._alf_sets(luma, chroma)
        self.alf_decide_dev(d_stats.ptr, n, d_luma.ptr, n_luma, d_chroma.ptr, n_chroma, lambda_q4, d_ctrl.ptr)
        return self._fetch((d_ctrl, np.uint8, (n, 3)))

    def alf_apply(self, tiles, w, h, luma, chroma, ctrl, classes=None, base=None):
        """numpy convenience around xAlfApplyGpu: a tile array, the packed sets, d_ctrl (uint8 [n_ctu, 3]) and a class map (None:
        classified inside) -> the filtered tile array; m_I, which the call does not write, comes from `base` (None: zeros)"""
        d_in, d_out = self._frame(tiles, w, h), self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        d_ctl, d_cls = self._table(ctrl, np.uint8, self.ctu_count(w, h) * 3), self._table(classes, np.uint8)
        d_luma, n_luma, d_chroma, n_chroma = self._alf_sets(luma, chroma)
        self.alf_apply_dev(d_in.ptr, w, h, d_cls.ptr, d_luma.ptr, n_luma, d_chroma.ptr, n_chroma, d_ctl.ptr, d_out.ptr)
        return self._fetch((d_out, np.uint8, (w * h * 2,)))

    def transform_ctu_from_tiles_dev(self, d_cur, d_pred, w, h, d_class, d_coef, stream=0):
        self._check(self.L.xTransformCtuFromTilesDev(self.ctx, d_cur, d_pred, w, h, d_class, d_coef, stream), "xTransformCtuFromTilesDev")

    def transform_ctu_to_tiles_dev(self, d_coef, d_class, d_pred, w, h, d_recon, stream=0):
        self._check(self.L.xTransformCtuToTilesDev(self.ctx, d_coef, d_class, d_pred, w, h, d_recon, stream), "xTransformCtuToTilesDev")

    @staticmethod
    def ctu_count(w, h):
        """CTUs of 64x64 that cover a w x h frame (the right and bottom ones possibly cut)"""
        return ((w + 63) // 64) * ((h + 63) // 64)

    def transform_ctu_from_tiles(self, cur_tiles, pred_tiles, w, h, classes):
        """numpy convenience around xTransformCtuFromTilesDev: two tile arrays of a w x h frame (uint8, 512 bytes per tile) and
        6 class bytes per CTU -> coefficients [n_ctus, 6, 1024] int16 (Y0 Y1 Y2 Y3 U V, each block-major for its class)."""
        n = self.ctu_count(w, h)
        dc, dp, dk, dz = self._frame(cur_tiles, w, h), self._frame(pred_tiles, w, h), self._table(classes, np.uint8, 6 * n), self.alloc(n * 12288)
        self.transform_ctu_from_tiles_dev(dc.ptr, dp.ptr, w, h, dk.ptr, dz.ptr)
        return self._fetch((dz, np.int16, (n, 6, 1024)))

    def transform_ctu_to_tiles(self, coef, classes, pred_tiles, w, h, base=None):
        """numpy convenience around xTransformCtuToTilesDev: coefficients [n_ctus, 6, 1024] int16, their class bytes and the pred
        tile array -> the reconstructed tile array; m_I (never written) comes from `base` (a tile array; None: pred's)."""
        n = self.ctu_count(w, h)
        dz, dk = self._table(coef, np.int16, n * 6144), self._table(classes, np.uint8, 6 * n)
        dp, dr = self._frame(pred_tiles, w, h), self._out_frame(base, pred_tiles)
        self.transform_ctu_to_tiles_dev(dz.ptr, dk.ptr, dp.ptr, w, h, dr.ptr)
        return self._fetch((dr, np.uint8, (w * h * 2,)))

    def quant_regions_dev(self, inverse, d_in, d_out, n_regions, d_class=0, d_qp=0, qp=0, rounding=0, d_nnz=0, stream=0):
        self._check(self.L.xQuantRegionsGpu(self.ctx, int(inverse), d_in, d_out, n_regions, d_class or None, d_qp or None, int(qp), int(rounding),
                                            d_nnz or None, stream), "xQuantRegionsGpu")

    def dct32_code_ctu_tiles_dev(self, d_cur, d_pred, w, h, d_qp, qp, rounding, d_level, d_nnz, d_recon, stream=0):
        self._check(self.L.xDct32CodeCtuTilesGpu(self.ctx, d_cur, d_pred, w, h, d_qp or None, int(qp), int(rounding), d_level, d_nnz or None, d_recon,
                                                 stream), "xDct32CodeCtuTilesGpu")

    def quant_regions(self, x, inverse=False, classes=None, qps=None, qp=0, rounding=0):
        """numpy convenience around xQuantRegionsGpu: [n_regions, 1024] int16, optional class and qp bytes per region -> the levels
        and their non-zero counts per region (inverse=False), or the coefficients (inverse=True)."""
        x = np.ascontiguousarray(x, np.int16).reshape(-1, 1024)
        n = x.shape[0]
        din, dout, dk, dq = self._upload(x), self.alloc(max(x.nbytes, 16)), self._table(classes, np.uint8, n), self._table(qps, np.uint8, n)
        dn = _NULL if inverse else self.alloc(max(4 * n, 16))
        self.quant_regions_dev(inverse, din.ptr, dout.ptr, n, dk.ptr, dq.ptr, qp, rounding, dn.ptr)
        out, nnz = self._fetch((dout, np.int16, (n, 1024)), (dn, np.uint32, (n,)))
        return out if inverse else (out, nnz)

    def code_ctu_tiles(self, cur_tiles, pred_tiles, w, h, qps=None, qp=0, rounding=0, base=None):
        """numpy convenience around xDct32CodeCtuTilesGpu: two tile arrays of a w x h frame (multiples of 64) and optionally 6 qp bytes per
        CTU -> (levels [n_ctus, 6, 1024] int16, non-zero counts [n_ctus, 6] uint32, the reconstructed tile array); m_I (never
        written) comes from `base` (a tile array; None: pred's)."""
        n = self.ctu_count(w, h)
        dc, dp, dr = self._frame(cur_tiles, w, h), self._frame(pred_tiles, w, h), self._out_frame(base, pred_tiles)
        dq, dl, dn = self._table(qps, np.uint8, 6 * n), self.alloc(n * 12288), self.alloc(max(n * 24, 16))
        self.dct32_code_ctu_tiles_dev(dc.ptr, dp.ptr, w, h, dq.ptr, qp, rounding, dl.ptr, dn.ptr, dr.ptr)
        return self._fetch((dl, np.int16, (n, 6, 1024)), (dn, np.uint32, (n, 6)), (dr, np.uint8, (w * h * 2,)))

    # -- the compact level stream -------------------------------------------------------------------
    @staticmethod
    def levels_params(d_level=0, d_class=0, d_nnz=0, d_region=0, d_stream=0, d_total=0, n_regions=0, cap_words=0):
        """an x266_levels_t from device addresses (0: NULL)"""
        return LevelsParams(d_level or None, d_class or None, d_nnz or None, d_region or None, d_stream or None, d_total or None, int(n_regions),
                            int(cap_words))

    def levels_pack_dev(self, params, stream=0):
        self._check(self.L.xLevelsPackGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xLevelsPackGpu")

    def levels_unpack_dev(self, params, stream=0):
        self._check(self.L.xLevelsUnpackGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xLevelsUnpackGpu")

    level_scan = staticmethod(level_scan)

    def levels_pack(self, levels, classes=None, nnz=None, cap_words=None):
        """numpy convenience around xLevelsPackGpu: [n_regions, 1024] int16 (and a class byte and a non-zero count per region, None:
        NULL) -> (records [n_regions] of LEVEL_REGION_DTYPE, stream uint16 [cap_words], total uint64 [2]).  cap_words None: a count-only
        call sizes the stream exactly; words the call does not write are 0."""
        x = np.ascontiguousarray(levels, np.int16).reshape(-1, 1024)
        n = x.shape[0]
        d_lv, d_rec, d_tot = self._upload(x), self.alloc(max(32 * n, 32)), self.alloc(16)
        d_cls, d_nnz = self._table(classes, np.uint8, n), self._table(nnz, np.uint32, n)
        p = self.levels_params(d_lv.ptr, d_cls.ptr, d_nnz.ptr, d_rec.ptr, 0, d_tot.ptr, n, 0)
        if cap_words is None:
            self.levels_pack_dev(p)
            cap_words = self._fetch((d_tot, np.uint64, (2,)))[0]
        cap_words = int(cap_words)
        d_str = self._upload(np.zeros(cap_words, np.uint16)) if cap_words else _NULL
        p.d_stream, p.cap_words = d_str.ptr or None, cap_words
        self.levels_pack_dev(p)
        return self._fetch((d_rec, LEVEL_REGION_DTYPE, (n,)), (d_str, np.uint16, (cap_words,)), (d_tot, np.uint64, (2,)))

    def levels_unpack(self, records, stream, n_regions, classes=None):
        """numpy convenience around xLevelsUnpackGpu: records (LEVEL_REGION_DTYPE), the stream's words and a class byte per region
        (None: NULL) -> (levels int16 [n_regions, 1024], non-zero counts uint32 [n_regions])"""
        n = int(n_regions)
        words = np.ascontiguousarray(stream, np.uint16).ravel()
        d_rec, d_cls = self._table(records, LEVEL_REGION_DTYPE, n),self._table(classes, np.uint8, n)
        d_str = self._upload(words) if words.size else _NULL
        d_lv, d_nnz = self.alloc(max(2048 * n, 16)), self.alloc(max(4 * n, 16))
        self.levels_unpack_dev(self.levels_params(d_lv.ptr, d_cls.ptr, d_nnz.ptr, d_rec.ptr, d_str.ptr, 0, n, words.size))
        return self._fetch((d_lv, np.int16, (n, 1024)), (d_nnz, np.uint32, (n,)))

    # -- RDOQ and the level rate estimate -----------------------------------------------------------------
    @staticmethod
    def rdoq_params(d_coef=0, d_level=0, d_class=0, d_qp=0, d_nnz=0, d_stat=0, n_regions=0, qp=0, lam=0):
        """an x266_rdoq_t from device addresses (0: NULL)"""
        return RdoqParams(d_coef or None, d_level or None, d_class or None, d_qp or None, d_nnz or None, d_stat or None, int(n_regions), int(qp), int(lam))

    def rdo_quant_dev(self, params, stream=0):
        self._check(self.L.xRdoQuantRegionsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xRdoQuantRegionsGpu")

    def levels_bits_dev(self, params, stream=0):
        self._check(self.L.xLevelsBitsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xLevelsBitsGpu")

    level_bits = staticmethod(level_bits)
    last_pos_bits = staticmethod(last_pos_bits)
    cg_flag_bits = staticmethod(cg_flag_bits)

    def rdo_quant(self, coef, classes=None, qps=None, qp=0, lam=368):
        """numpy convenience around xRdoQuantRegionsGpu: [n_regions, 1024] int16, optional class and qp bytes per region -> (levels int16
        [n_regions, 1024], non-zero counts uint32 [n_regions], records [n_regions] of RDOQ_REGION_DTYPE)"""
        x = np.ascontiguousarray(coef, np.int16).reshape(-1, 1024)
        n = x.shape[0]
        d_in, d_cls, d_qp = self._upload(x), self._table(classes, np.uint8, n), self._table(qps, np.uint8, n)
        d_out, d_nnz, d_stat = self.alloc(max(x.nbytes, 16)), self.alloc(max(4 * n, 16)), self.alloc(max(16 * n, 16))
        self.rdo_quant_dev(self.rdoq_params(d_in.ptr, d_out.ptr, d_cls.ptr, d_qp.ptr, d_nnz.ptr, d_stat.ptr, n, qp, lam))
        return self._fetch((d_out, np.int16, (n, 1024)), (d_nnz, np.uint32, (n,)), (d_stat, RDOQ_REGION_DTYPE, (n,)))

    def levels_bits(self, levels, classes=None, nnz=None):
        """numpy convenience around xLevelsBitsGpu: [n_regions, 1024] int16 (and a class byte and a non-zero count per region, None: NULL)
        -> records [n_regions] of RDOQ_REGION_DTYPE (dist 0)"""
        x = np.ascontiguousarray(levels, np.int16).reshape(-1, 1024)
        n = x.shape[0]
        d_lv, d_cls, d_nnz, d_stat = self._upload(x), self._table(classes, np.uint8, n), self._table(nnz, np.uint32, n), self.alloc(max(16 * n, 16))
        self.levels_bits_dev(self.rdoq_params(0, d_lv.ptr, d_cls.ptr, 0, d_nnz.ptr, d_stat.ptr, n))
        return self._fetch((d_stat, RDOQ_REGION_DTYPE, (n,)))

    # -- the transform decision: each region's class byte by rate-distortion cost ------------------------
    @staticmethod
    def tdecide_params(d_cur=0, d_pred=0, d_qp=0, d_cand=0, d_class=0, d_level=0, d_nnz=0, d_stat=0, d_cost=0, width=0, height=0, qp=0, lam=0,
                       cand_luma=TDECIDE_CLASSES, cand_chroma=TDECIDE_CLASSES, class_bits=None):
        """an x266_tdecide_t from device addresses (0: NULL); class_bits: up to 16 values in 1/16 bit (None: zeros)"""
        bits = (ctypes.c_uint16 * 16)(*[int(b) for b in (class_bits if class_bits is not None else ())])
        return TDecideParams(d_cur or None, d_pred or None, d_qp or None, d_cand or None, d_class or None, d_level or None, d_nnz or None,
                             d_stat or None, d_cost or None, int(width), int(height), int(qp), int(lam), int(cand_luma), int(cand_chroma), bits)

    def transform_decide_dev(self, params, stream=0):
        self._check(self.L.xTransformDecideCtuTilesGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream),
                    "xTransformDecideCtuTilesGpu")

    def transform_decide(self, cur_tiles, pred_tiles, w, h, qps=None, qp=0, lam=368, cand_luma=TDECIDE_CLASSES, cand_chroma=TDECIDE_CLASSES,
                         cand=None, class_bits=None):
        """numpy convenience around xTransformDecideCtuTilesGpu: two tile arrays of a w x h frame (uint8, 512 bytes per tile), optional qp
        bytes and candidate masks (uint16) per region -> (class bytes uint8 [n], levels int16 [n, 1024], non-zero counts uint32 [n],
        records [n] of RDOQ_REGION_DTYPE, costs uint64 [n, 16]) with n = 6 CTUs' regions."""
        n = 6 * self.ctu_count(w, h)
        dc, dp, d_qp, d_cand = self._frame(cur_tiles, w, h), self._frame(pred_tiles, w, h), self._table(qps, np.uint8, n), self._table(cand, np.uint16, n)
        d_cls, d_lv, d_nnz, d_stat, d_cost = self.alloc(max(n, 16)), self.alloc(n * 2048), self.alloc(max(4 * n, 16)), self.alloc(16 * n), self.alloc(128 * n)
        self.transform_decide_dev(self.tdecide_params(dc.ptr, dp.ptr, d_qp.ptr, d_cand.ptr, d_cls.ptr, d_lv.ptr, d_nnz.ptr, d_stat.ptr, d_cost.ptr,
                                                      w, h, qp, lam, cand_luma, cand_chroma, class_bits))
        return self._fetch((d_cls, np.uint8, (n,)), (d_lv, np.int16, (n, 1024)), (d_nnz, np.uint32, (n,)), (d_stat, RDOQ_REGION_DTYPE, (n,)),
                           (d_cost, np.uint64, (n, 16)))

    # -- source analysis: tile activity, the qp map, fade weights ---------------------------------------
    @staticmethod
    def aq_params(d_src=0, d_tile=0, d_total=0, d_offset=0, d_qp=0, width=0, height=0, mode=1, strength_q8=256, qp=0, chroma_qp_offset=0):
        """an x266_aq_t from device addresses (0: NULL)"""
        return AqParams(d_src or None, d_tile or None, d_total or None, d_offset or None, d_qp or None, int(width), int(height), int(mode), int(strength_q8),
                        int(qp), int(chroma_qp_offset))

    def aq_stats_dev(self, params, stream=0):
        self._check(self.L.xAqStatsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xAqStatsGpu")

    def aq_decide_dev(self, params, stream=0):
        self._check(self.L.xAqDecideGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xAqDecideGpu")

    def aq_stats(self, tiles, w, h):
        """numpy convenience around xAqStatsGpu: the tile array of a w x h frame -> (records [n_tiles] of AQ_TILE_DTYPE, totals int64 [8])"""
        n = (w // 16) * (h // 16)
        d_src, d_tile, d_total = self._frame(tiles, w, h), self.alloc(32 * n), self.alloc(64)
        self.aq_stats_dev(self.aq_params(d_src.ptr, d_tile.ptr, d_total.ptr, width=w, height=h))
        return self._fetch((d_tile, AQ_TILE_DTYPE, (n,)), (d_total, np.int64, (8,)))

    def aq_decide(self, records, totals, w, h, mode=1, strength_q8=256, qp=32, chroma_qp_offset=0):
        """numpy convenience around xAqDecideGpu: the records and totals of aq_stats -> (Q8 offsets int16 [n_tiles], qp bytes uint8 [n_ctus, 6])"""
        n, n_ctu = (w // 16) * (h // 16), self.ctu_count(w, h)
        d_tile, d_total = self._table(records, AQ_TILE_DTYPE, n), self._table(totals, np.int64, 8)
        d_off, d_qp = self.alloc(max(2 * n, 16)), self.alloc(max(6 * n_ctu, 16))
        self.aq_decide_dev(self.aq_params(0, d_tile.ptr, d_total.ptr, d_off.ptr, d_qp.ptr, w, h, mode, strength_q8, qp, chroma_qp_offset))
        return self._fetch((d_off, np.int16, (n,)), (d_qp, np.uint8, (n_ctu, 6)))

    @staticmethod
    def weights_from_totals(cur, ref, lst=0, log2_denom=(7, 7), wp=None):
        """xWeightsFromTotals (host, no device): the totals of the current and of the reference frame -> the wp_params object of the
        bi-directional methods with w[lst] and o[lst] estimated; wp None: a fresh one whose other list holds the default weights at
        log2_denom (127, the largest weight, at a denominator of 7)"""
        if wp is None:
            one = [min(1 << min(int(log2_denom[0]), 7), 127)] + [min(1 << min(int(log2_denom[1]), 7), 127)] * 2
            wp = Codec.wp_params(w=(one, one), log2_denom=log2_denom)
        c, r = np.ascontiguousarray(cur, np.int64), np.ascontiguousarray(ref, np.int64)
        if c.size != 8 or r.size != 8 or load_library().xWeightsFromTotals(_P(c.ctypes.data), _P(r.ctypes.data), int(lst), ctypes.byref(wp)) != 0:
            raise X266Error("xWeightsFromTotals: list must be 0 or 1, log2_denom 0..7, and the totals those of two frames of one size")
        return wp

    # -- frame quality: SSE and SSIM per CTU and per frame (the numpy calls are x266_amd.quality's) ---------
    def quality_stats_dev(self, params, stream=0):
        self._check(self.L.xQualityStatsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xQualityStatsGpu")

    # -- the lookahead: half-size frames, frame costs, the propagation tree --------------------------------
    @staticmethod
    def la_params(width=0, height=0, intra_penalty=0, strength_q8=256, qp=0, chroma_qp_offset=0, **pointers):
        """an x266_la_t from device addresses by field name (absent or 0: NULL)"""
        return Codec._keyword_params(LaParams, "la_params", pointers, (width, height, intra_penalty, strength_q8, qp, chroma_qp_offset))

    def _la_dev(self, call, params, stream):
        self._check(getattr(self.L, LA_CALLS[call])(self.ctx, ctypes.byref(params) if params is not None else None, stream), LA_CALLS[call])

    def la_downscale_dev(self, params, stream=0):
        self._la_dev("downscale", params, stream)

    def la_intra_costs_dev(self, params, stream=0):
        self._la_dev("intra_costs", params, stream)

    def la_frame_cost_dev(self, params, stream=0):
        self._la_dev("frame_cost", params, stream)

    def la_propagate_dev(self, params, stream=0):
        self._la_dev("propagate", params, stream)

    def la_tree_qp_dev(self, params, stream=0):
        self._la_dev("tree_qp", params, stream)

    def la_downscale(self, tiles, w, h):
        """numpy convenience around xLaDownscaleGpu: the tile array of a w x h frame -> the lowres tile array [n / 4, 512] (m_I zero)"""
        d_src, d_low = self._frame(tiles, w, h), self._upload(np.zeros(w * h // 2, np.uint8))
        self.la_downscale_dev(self.la_params(w, h, d_src=d_src.ptr, d_low=d_low.ptr))
        return self._fetch((d_low, np.uint8, (w * h // 1024, 512)))

    def la_intra_costs(self, low_tiles, w, h):
        """numpy convenience around xLaIntraCostsGpu: the lowres tile array of a w x h frame -> (costs uint32 [n], modes uint8 [n])"""
        n = (w // 16) * (h // 16)
        d_low, d_intra, d_mode = self._table(low_tiles, np.uint8, w * h // 2), self.alloc(4 * n), self.alloc(max(n, 16))
        self.la_intra_costs_dev(self.la_params(w, h, d_low=d_low.ptr, d_intra=d_intra.ptr, d_mode=d_mode.ptr))
        return self._fetch((d_intra, np.uint32, (n,)), (d_mode, np.uint8, (n,)))

    def la_frame_cost(self, intra, mode, inter0, inter1, w, h, intra_penalty=0):
        """numpy convenience around xLaFrameCostGpu: intra costs, modes (or None) and the lists' search records (8 bytes each, or None)
        -> (records [n] of LA_BLOCK_DTYPE, totals int64 [8])"""
        n = (w // 16) * (h // 16)
        d_intra, d_mode, d_in0, d_in1 = self._table(intra, np.uint32), self._table(mode, np.uint8), self._table(inter0, None), self._table(inter1, None)
        assert d_intra and d_intra.nbytes >= 4 * n
        d_block, d_total = self.alloc(16 * n), self.alloc(64)
        self.la_frame_cost_dev(self.la_params(w, h, intra_penalty, d_intra=d_intra.ptr, d_mode=d_mode.ptr, d_inter0=d_in0.ptr, d_inter1=d_in1.ptr,
                                              d_block=d_block.ptr, d_total=d_total.ptr))
        return self._fetch((d_block, LA_BLOCK_DTYPE, (n,)), (d_total, np.int64, (8,)))

    def la_propagate(self, records, prop, ref0, ref1, w, h):
        """numpy convenience around xLaPropagateGpu: the records, what the frame received (uint64 [n] or None) and the two
        accumulators as they stand (uint64 [n] or None) -> the two accumulators after the step (None stays None)"""
        n = (w // 16) * (h // 16)
        d_block, (d_prop, d_r0, d_r1) = self._table(records, LA_BLOCK_DTYPE), (self._table(a, np.uint64) for a in (prop, ref0, ref1))
        self.la_propagate_dev(self.la_params(w, h, d_block=d_block.ptr, d_prop=d_prop.ptr, d_prop_ref0=d_r0.ptr, d_prop_ref1=d_r1.ptr))
        return list(self._fetch((d_r0, np.uint64, (n,)), (d_r1, np.uint64, (n,))))

    def la_tree_qp(self, records, prop, aq_offset, w, h, strength_q8=256, qp=32, chroma_qp_offset=0):
        """numpy convenience around xLaTreeQpGpu: the records, what the frame received and the AQ offsets (either may be None)
        -> (Q8 offsets int16 [n], qp bytes uint8 [n_ctus, 6])"""
        n, n_ctu = (w // 16) * (h // 16), self.ctu_count(w, h)
        d_block, d_prop, d_aq = self._table(records, LA_BLOCK_DTYPE), self._table(prop, np.uint64), self._table(aq_offset, np.int16)
        d_off, d_qp = self.alloc(max(2 * n, 16)), self.alloc(max(6 * n_ctu, 16))
        self.la_tree_qp_dev(self.la_params(w, h, 0, strength_q8, qp, chroma_qp_offset, d_block=d_block.ptr, d_prop=d_prop.ptr, d_aq_offset=d_aq.ptr,
                                           d_offset=d_off.ptr, d_qp=d_qp.ptr))
        return self._fetch((d_off, np.int16, (n,)), (d_qp, np.uint8, (n_ctu, 6)))

    # -- the seeded search: a small SATD search around per-block starting vectors ------------------------------
    @staticmethod
    def seed_params(width=0, height=0, seed_scale=0, centres=0, range=0, lambda_q4=0, **pointers):
        """an x266_seed_t from device addresses by field name (absent or 0: NULL)"""
        return Codec._keyword_params(SeedParams, "seed_params", pointers, (width, height, seed_scale, centres, range, lambda_q4))

    def satd_seeded_search_dev(self, params, stream=0):
        self._check(self.L.xSatd8x8SeededSearchGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xSatd8x8SeededSearchGpu")

    def seeded_search_tiles(self, cur_tiles, ref_tiles, w, h, seeds, seed_scale=0, centres=0, rng=0, lambda_q4=0):
        """numpy convenience around xSatd8x8SeededSearchGpu: two tile arrays of a w x h frame and the seed vectors [cells, 2] int16
        -> (mv [nb, 2] int16, satd [nb] uint32, j [nb] uint32)"""
        nb = (h // 8) * (w // 8)
        dc, dr, ds = self._frame(cur_tiles, w, h), self._frame(ref_tiles, w, h), self._upload(self._records(seeds, nb >> (2 * seed_scale)))
        db, dj = self.alloc(nb * 8), self.alloc(max(nb * 4, 16))
        self.satd_seeded_search_dev(self.seed_params(w, h, seed_scale, centres, rng, lambda_q4, d_cur=dc.ptr, d_ref=dr.ptr, d_seed=ds.ptr, d_best=db.ptr, d_j=dj.ptr))
        return self._fetch_best(db, nb, dj, (nb,))

    # -- the inter partition decision: the numpy calls are x266_amd/partition.py's ------------------------------
    def inter_partition_decide_dev(self, params, stream=0):
        self._check(self.L.xInterPartitionDecideGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xInterPartitionDecideGpu")

    # -- the compact motion stream: the numpy calls and the host helpers are x266_amd/motion.py's -----------------
    def motion_pack_dev(self, params, stream=0):
        self._check(self.L.xMotionPackGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xMotionPackGpu")

    def motion_unpack_dev(self, params, stream=0):
        self._check(self.L.xMotionUnpackGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xMotionUnpackGpu")

    # -- the entropy coder of the level stream: the numpy calls and the host helpers are x266_amd/entropy.py's ----
    def entropy_encode_levels_dev(self, params, stream=0):
        self._check(self.L.xEntropyEncodeLevelsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyEncodeLevelsGpu")

    def entropy_decode_levels_dev(self, params, stream=0):
        self._check(self.L.xEntropyDecodeLevelsGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyDecodeLevelsGpu")

    # -- the vectors from the differences: the numpy call is x266_amd/motion.py's; the coder of the motion stream is x266_amd/entropy.py's ----
    def motion_reconstruct_dev(self, params, stream=0):
        self._check(self.L.xMotionReconstructGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xMotionReconstructGpu")

    # -- mixed inter / intra coding of a frame: intra 32x32 regions in P- and B-frames -------------------------
    @staticmethod
    def mixed_params(width=0, height=0, qp=0, rounding=0, intra_penalty=0, **pointers):
        """an x266_mixed_t from device addresses by field name (absent or 0: NULL)"""
        return Codec._keyword_params(MixedParams, "mixed_params", pointers, (width, height, qp, rounding, intra_penalty))

    def dct32_code_mixed_frame_dev(self, params, stream=0):
        self._check(self.L.xDct32CodeMixedFrameGpu(self.ctx, ctypes.byref(params) if params is not None else None, stream), "xDct32CodeMixedFrameGpu")

    def code_mixed_frame(self, cur_tiles, pred_tiles, w, h, qps=None, qp=0, rounding=0, intra_penalty=0, kinds_in=None, modes_in=None, base=None):
        """numpy convenience around xDct32CodeMixedFrameGpu: two tile arrays of a w x h frame (multiples of 64), optionally 6 qp, kind and
        mode bytes per CTU -> a dict of levels [n_ctus, 6, 1024] int16, nnz [n_ctus, 6] uint32, kinds and modes [n_ctus, 6] uint8, costs
        [n_ctus, 6, 2] uint32 (inter, intra) and the reconstructed tile array; m_I (never written) comes from `base` (None: zeros)"""
        n = self.ctu_count(w, h)
        dc, dp, dr = self._frame(cur_tiles, w, h), self._frame(pred_tiles, w, h), self._out_frame(base, np.zeros(w * h * 2, np.uint8))
        dq, dki, dmi = (self._table(t, np.uint8, 6 * n, tail=16) for t in (qps, kinds_in, modes_in))
        dl, dn, dk, dm, dcost = self.alloc(n * 12288), self.alloc(max(n * 24, 16)), self.alloc(max(n * 6, 16)), self.alloc(max(n * 6, 16)), self.alloc(n * 48)
        self.dct32_code_mixed_frame_dev(self.mixed_params(w, h, qp, rounding, intra_penalty, d_cur=dc.ptr, d_pred=dp.ptr, d_qp=dq.ptr, d_kind_in=dki.ptr,
                                                          d_mode_in=dmi.ptr, d_level=dl.ptr, d_nnz=dn.ptr, d_kind=dk.ptr, d_mode=dm.ptr, d_cost=dcost.ptr,
                                                          d_recon=dr.ptr))
        got = self._fetch((dl, np.int16, (n, 6, 1024)), (dn, np.uint32, (n, 6)), (dk, np.uint8, (n, 6)), (dm, np.uint8, (n, 6)), (dcost, np.uint32, (n, 6, 2)),
                          (dr, np.uint8, (w * h * 2,)))
        return dict(zip(("levels", "nnz", "kinds", "modes", "costs", "recon"), got))

    def fill_residual_dev(self, d_dst, n_samples, seed, first_index=0, stream=0):
        self._check(self.L.xFillResidualDev(self.ctx, d_dst, n_samples, seed, first_index, stream),
                    "xFillResidualDev")

    # -- streams and graphs (for launch-bound sequences) ---------------------------------------
    def stream_create(self):
        s = _P()
        self._check(self.L.xHipStreamCreate(self.ctx, ctypes.byref(s)), "xHipStreamCreate")
        return s.value

    def stream_destroy(self, stream):
        self._check(self.L.xHipStreamDestroy(self.ctx, stream), "xHipStreamDestroy")

    def graph_begin(self, stream):
        self._check(self.L.xHipGraphBegin(self.ctx, stream), "xHipGraphBegin")

    def graph_end(self, stream):
        g = _P()
        self._check(self.L.xHipGraphEnd(self.ctx, stream, ctypes.byref(g)), "xHipGraphEnd")
        return g.value

    def graph_launch(self, graph, stream):
        self._check(self.L.xHipGraphLaunch(self.ctx, graph, stream), "xHipGraphLaunch")

    def graph_free(self, graph):
        self.L.xHipGraphFree(self.ctx, graph)

    def stream_sync(self, stream=0):
        self._check(self.L.xHipStreamSync(self.ctx, stream), "xHipStreamSync")

    def time_kernel(self, op, d_in, d_out, n_blocks, reps, stream=0):
        ms = ctypes.c_double()
        self._check(self.L.xHipTimeKernel(self.ctx, op, d_in, d_out, n_blocks, reps, stream, ctypes.byref(ms)),
                    "xHipTimeKernel")
        return ms.value

    # -- HIP events on the launching stream (per-launch durations of any sequence of calls) -------
    def event_create(self):
        e = _P()
        self._check(self.L.xHipEventCreate(self.ctx, ctypes.byref(e)), "xHipEventCreate")
        return e.value

    def event_destroy(self, event):
        self._check(self.L.xHipEventDestroy(self.ctx, event), "xHipEventDestroy")

    def event_record(self, event, stream=0):
        self._check(self.L.xHipEventRecord(self.ctx, event, stream), "xHipEventRecord")

    def event_elapsed_ms(self, start, stop):
        ms = ctypes.c_double()
        self._check(self.L.xHipEventElapsedMs(self.ctx, start, stop, ctypes.byref(ms)), "xHipEventElapsedMs")
        return ms.value

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def host_alloc(self, shape, dtype):
        """A numpy array in page-locked host memory (xHipHostAlloc): the host-pointer batch calls move it by DMA (43 GB/s each way
        instead of 27 from pageable memory).  The allocation belongs to a buffer owner at the END of the base chain of the array
        and of every view, slice or reshape of it: it is freed when the last of them is gone, never under a live view.  A context
        closed while blocks are alive is freed with the last block."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        nbytes = max(n * dtype.itemsize, 1)
        p = _P()
        self._check(self.L.xHipHostAlloc(self.ctx, ctypes.byref(p), nbytes), "xHipHostAlloc")
        owner = _PinnedBlock(self, p.value, nbytes)
        return np.asarray(owner)[: n * dtype.itemsize].view(dtype).reshape(shape)


class _PinnedBlock:
    """Owner of one pinned allocation: numpy takes the memory through __array_interface__ and keeps this object as the base of
    the array it builds, so every view's base chain ends here (a finalizer on ONE ndarray fired under live views)."""

    def __init__(self, codec, ptr, nbytes):
        self.codec, self.ptr, self.nbytes = codec, ptr, nbytes
        with codec._lock():                                             # __del__ below may run on any thread (GC)
            codec._pinned_live = getattr(codec, "_pinned_live", 0) + 1
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def __del__(self):
        codec, ptr = self.codec, self.ptr
        self.ptr = 0
        if not ptr or codec is None:
            return
        try:
            with codec._lock():
                ctx = getattr(codec, "ctx", None) or getattr(codec, "_ctx_for_free", None)
                if ctx:
                    codec.L.xHipHostFree(ctx, ptr)
                codec._pinned_live -= 1
                if codec._pinned_live == 0 and codec.close_deferred:
                    codec.close()
        except Exception:
            pass
