"""x266_amd -- thin Python binding (ctypes) over libx266hip.so, the MI355X
implementation of x266's DCT32 / SATD hot path.

The product is the C-ABI shared library (include/x266hip.h); this module only
exists so that Python hosts (tests, bench.py) can call the same entry points a
C/C++ host would.  It contains no arithmetic and no fallback: if the library
or a gfx950 device is missing, calls raise.
"""
from ._lib import (X266Error, Codec, lib_path, load_library, build_library,  # noqa: F401
                   pack_diff_rows, pack_dct_word, LevelsParams, LEVEL_REGION_DTYPE, level_scan, levels_scan_chunk,
                   RdoqParams, RDOQ_REGION_DTYPE, level_bits, last_pos_bits, cg_flag_bits, TDecideParams, TDECIDE_CLASSES,
                   AqParams, AQ_TILE_DTYPE, aq_totals_chunk, QualityParams, QUALITY_CTU_DTYPE, QUALITY_SSE, QUALITY_SSIM,
                   LaParams, LA_BLOCK_DTYPE, la_totals_chunk, scene_cut_from_totals, SeedParams, MixedParams, PartParams, PART_CTU_DTYPE,
                   MotionParams, MOTION_CTU_DTYPE, EntropyParams, ENTROPY_REGION_DTYPE, ENTROPY_CONTEXTS, ENTROPY_MAX_BYTES,
                   EntropyMotionParams, ENTROPY_MOTION_CTU_DTYPE, ENTROPY_MOTION_CONTEXTS, ENTROPY_MOTION_MAX_BYTES,
                   EntropySideParams, ENTROPY_SIDE_CTU_DTYPE, ENTROPY_SIDE_CONTEXTS, ENTROPY_SIDE_MAX_BYTES,
                   EntropyStatsParams, EntropySideStatsParams, ENTROPY_STATS_REGIONS, ENTROPY_SIDE_STATS_CTUS)

__all__ = ["X266Error", "Codec", "lib_path", "load_library", "build_library",
           "pack_diff_rows", "pack_dct_word", "LevelsParams", "LEVEL_REGION_DTYPE", "level_scan", "levels_scan_chunk",
           "RdoqParams", "RDOQ_REGION_DTYPE", "level_bits", "last_pos_bits", "cg_flag_bits", "TDecideParams", "TDECIDE_CLASSES",
           "AqParams", "AQ_TILE_DTYPE", "aq_totals_chunk", "QualityParams", "QUALITY_CTU_DTYPE", "QUALITY_SSE", "QUALITY_SSIM",
           "LaParams", "LA_BLOCK_DTYPE", "la_totals_chunk", "scene_cut_from_totals", "SeedParams", "MixedParams", "PartParams", "PART_CTU_DTYPE",
           "MotionParams", "MOTION_CTU_DTYPE", "EntropyParams", "ENTROPY_REGION_DTYPE", "ENTROPY_CONTEXTS", "ENTROPY_MAX_BYTES",
           "EntropyMotionParams", "ENTROPY_MOTION_CTU_DTYPE", "ENTROPY_MOTION_CONTEXTS", "ENTROPY_MOTION_MAX_BYTES",
           "EntropySideParams", "ENTROPY_SIDE_CTU_DTYPE", "ENTROPY_SIDE_CONTEXTS", "ENTROPY_SIDE_MAX_BYTES",
           "EntropyStatsParams", "EntropySideStatsParams", "ENTROPY_STATS_REGIONS", "ENTROPY_SIDE_STATS_CTUS"]
