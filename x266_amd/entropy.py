"""The entropy coder of the level stream (include/x266hip.h: xEntropyEncodeLevelsGpu, xEntropyDecodeLevelsGpu): the numpy calls around
Codec.entropy_encode_levels_dev and Codec.entropy_decode_levels_dev, built from the pieces the Codec's own numpy methods are built from,
and the three host helpers of the library (xEntropyDefaultInit, xEntropyEncodeRegion, xEntropyDecodeRegion); below them the same for the
motion stream (xEntropyEncodeMvGpu, xEntropyDecodeMvGpu and their three helpers) and for the side information (xEntropyEncodeSideGpu,
xEntropyDecodeSideGpu and their three helpers), and at the end the per-context bin statistics (xEntropyStatsLevelsGpu, xEntropyStatsSideGpu,
xEntropyInitFromCounts and the two counting helpers).  No arithmetic lives here."""
import ctypes

import numpy as np

from ._lib import (ENTROPY_CONTEXTS, ENTROPY_MAX_BYTES, ENTROPY_MOTION_CONTEXTS, ENTROPY_MOTION_CTU_DTYPE, ENTROPY_MOTION_MAX_BYTES, ENTROPY_REGION_DTYPE,
                   ENTROPY_SIDE_CONTEXTS, ENTROPY_SIDE_CTU_DTYPE, ENTROPY_SIDE_MAX_BYTES, MOTION_CTU_DTYPE, Codec, EntropyMotionParams, EntropyParams,
                   ENTROPY_SIDE_STATS_CTUS, ENTROPY_STATS_REGIONS, EntropySideParams, EntropySideStatsParams, EntropyStatsParams, X266Error, _NULL, load_library)


def _init_table(init):
    """the host table a call reads: None stays None (the default); the array must outlive the call, so it is returned"""
    if init is None:
        return None
    table = np.ascontiguousarray(init, np.uint16).ravel()
    if table.size != ENTROPY_CONTEXTS:
        raise X266Error("init must hold %d entries" % ENTROPY_CONTEXTS)
    return table


def entropy_params(**fields):
    """an x266_entropy_t by field name: device addresses (absent or 0: NULL) and the HOST address `init`, then n_regions and cap_words"""
    scalars = [fields.pop("n_regions", 0), fields.pop("cap_words", 0)]
    return Codec._keyword_params(EntropyParams, "entropy_params", fields, scalars)


def entropy_encode_levels(codec, levels, classes=None, nnz=None, cap_words=None, init=None):
    """numpy convenience around xEntropyEncodeLevelsGpu: [n_regions, 1024] int16 (and a class byte and a non-zero count per region, None:
    NULL; init: 100 uint16 or None) -> (records [n_regions] of ENTROPY_REGION_DTYPE, stream uint16 [cap_words], total uint64 [2]).
    cap_words None: a count-only call sizes the stream exactly; words the call does not write are 0."""
    lv = np.ascontiguousarray(levels, np.int16).reshape(-1, 1024)
    n = lv.shape[0]
    table = _init_table(init)
    d_level = codec._upload(lv)
    d_class, d_nnz = codec._table(classes, np.uint8, n), codec._table(nnz, np.uint32, n)
    d_region, d_tot = codec.alloc(max(32 * n, 16)), codec.alloc(16)
    p = entropy_params(d_level=d_level.ptr, d_class=d_class.ptr, d_nnz=d_nnz.ptr, d_region=d_region.ptr, d_total=d_tot.ptr,
                       init=table.ctypes.data if table is not None else 0, n_regions=n)
    if cap_words is None:
        codec.entropy_encode_levels_dev(p)
        cap_words = codec._fetch((d_tot, np.uint64, (2,)))[0]
    cap_words = int(cap_words)
    d_str = codec._upload(np.zeros(cap_words, np.uint16)) if cap_words else _NULL
    p.d_stream, p.cap_words = d_str.ptr or None, cap_words
    codec.entropy_encode_levels_dev(p)
    return codec._fetch((d_region, ENTROPY_REGION_DTYPE, (n,)), (d_str, np.uint16, (cap_words,)), (d_tot, np.uint64, (2,)))


def entropy_decode_levels(codec, records, stream, classes=None, init=None):
    """numpy convenience around xEntropyDecodeLevelsGpu: records (ENTROPY_REGION_DTYPE) and the stream's words -> (levels [n_regions, 1024]
    int16, nnz [n_regions] uint32)"""
    rec = np.ascontiguousarray(records, ENTROPY_REGION_DTYPE).ravel()
    n = rec.size
    words = np.ascontiguousarray(stream, np.uint16).ravel()
    table = _init_table(init)
    d_region = codec._upload(rec)
    d_str = codec._upload(words) if words.size else _NULL
    d_class = codec._table(classes, np.uint8, n)
    d_level, d_nnz = codec.alloc(max(2048 * n, 16)), codec.alloc(max(4 * n, 16))
    codec.entropy_decode_levels_dev(entropy_params(d_level=d_level.ptr, d_class=d_class.ptr, d_nnz=d_nnz.ptr, d_region=d_region.ptr, d_stream=d_str.ptr,
                                                   init=table.ctypes.data if table is not None else 0, n_regions=n, cap_words=words.size))
    return codec._fetch((d_level, np.int16, (n, 1024)), (d_nnz, np.uint32, (n,)))


# ---- the host helpers: the library's own functions, no device ------------------------------------------------------------------------------
def entropy_default_init():
    """xEntropyDefaultInit: the default table, 100 uint16"""
    table = np.zeros(ENTROPY_CONTEXTS, np.uint16)
    if load_library().xEntropyDefaultInit(table.ctypes.data) != 0:
        raise X266Error("xEntropyDefaultInit failed")
    return table


def entropy_encode_region(level, cls=3, init=None, cap=ENTROPY_MAX_BYTES):
    """xEntropyEncodeRegion: (the substream's first min(n_bytes, cap) bytes, n_bytes, context bins, bypass bins)"""
    lv = np.ascontiguousarray(level, np.int16).ravel()
    if lv.size != 1024:
        raise X266Error("a region is 1024 levels")
    table = _init_table(init)
    out, bins = np.zeros(max(int(cap), 1), np.uint8), np.zeros(2, np.uint32)
    n = load_library().xEntropyEncodeRegion(lv.ctypes.data, int(cls), table.ctypes.data if table is not None else None, out.ctypes.data if cap else None, int(cap),
                                            bins.ctypes.data)
    if n < 0:
        raise X266Error("xEntropyEncodeRegion: a bad argument")
    return out[:min(n, int(cap))].tobytes(), n, int(bins[0]), int(bins[1])


def entropy_decode_region(data, cls=3, init=None):
    """xEntropyDecodeRegion: (levels [1024] int16, n_nz, malformed)"""
    raw = np.frombuffer(bytes(data), np.uint8)
    table = _init_table(init)
    level, n_nz = np.zeros(1024, np.int16), np.zeros(1, np.uint32)
    rc = load_library().xEntropyDecodeRegion(raw.ctypes.data if raw.size else None, raw.size, int(cls), table.ctypes.data if table is not None else None,
                                             level.ctypes.data, n_nz.ctypes.data)
    if rc < 0:
        raise X266Error("xEntropyDecodeRegion: a bad argument")
    return level, int(n_nz[0]), rc == 1


# ---- the motion stream (xEntropyEncodeMvGpu, xEntropyDecodeMvGpu) -----------------------------------------------------------------------
def _motion_table(init):
    if init is None:
        return None
    table = np.ascontiguousarray(init, np.uint16).ravel()
    if table.size != ENTROPY_MOTION_CONTEXTS:
        raise X266Error("init must hold %d entries" % ENTROPY_MOTION_CONTEXTS)
    return table


def entropy_motion_params(**fields):
    """an x266_entropy_motion_t by field name: device addresses (absent or 0: NULL) and the HOST address `init`, then width, height, in_words
    and cap_words"""
    scalars = [fields.pop("width", 0), fields.pop("height", 0), fields.pop("in_words", 0), fields.pop("cap_words", 0)]
    return Codec._keyword_params(EntropyMotionParams, "entropy_motion_params", fields, scalars)


def entropy_encode_motion_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyEncodeMvGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyEncodeMvGpu")


def entropy_decode_motion_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyDecodeMvGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyDecodeMvGpu")


def entropy_encode_motion(codec, records, words, w, h, cap_words=None, init=None):
    """numpy convenience around xEntropyEncodeMvGpu: the records (MOTION_CTU_DTYPE) and the words of xMotionPackGpu for a w x h frame
    (init: 7 uint16 or None) -> (coded [n_ctu] of ENTROPY_MOTION_CTU_DTYPE, stream uint16 [cap_words], total uint64 [2]).  cap_words None: a
    count-only call sizes the stream exactly; words the call does not write are 0."""
    n_ctu = codec.ctu_count(w, h)
    src = np.ascontiguousarray(words, np.uint16).ravel()
    table = _motion_table(init)
    d_ctu = codec._table(records, MOTION_CTU_DTYPE, n_ctu)
    d_words = codec._upload(src) if src.size else _NULL
    d_coded, d_tot = codec.alloc(32 * n_ctu), codec.alloc(16)
    p = entropy_motion_params(d_ctu=d_ctu.ptr, d_words=d_words.ptr, d_coded=d_coded.ptr, d_total=d_tot.ptr, init=table.ctypes.data if table is not None else 0,
                              width=w, height=h, in_words=src.size)
    if cap_words is None:
        entropy_encode_motion_dev(codec, p)
        cap_words = codec._fetch((d_tot, np.uint64, (2,)))[0]
    cap_words = int(cap_words)
    d_str = codec._upload(np.zeros(cap_words, np.uint16)) if cap_words else _NULL
    p.d_stream, p.cap_words = d_str.ptr or None, cap_words
    entropy_encode_motion_dev(codec, p)
    return codec._fetch((d_coded, ENTROPY_MOTION_CTU_DTYPE, (n_ctu,)), (d_str, np.uint16, (cap_words,)), (d_tot, np.uint64, (2,)))


def entropy_decode_motion(codec, coded, stream, w, h, init=None):
    """numpy convenience around xEntropyDecodeMvGpu: the coded records (ENTROPY_MOTION_CTU_DTYPE) and the stream's words of a w x h frame ->
    (records [n_ctu] of MOTION_CTU_DTYPE, words uint16 [256 * n_ctu] -- zero where the call writes nothing --, status uint8 [n_ctu])"""
    n_ctu = codec.ctu_count(w, h)
    src = np.ascontiguousarray(stream, np.uint16).ravel()
    table = _motion_table(init)
    d_coded = codec._table(coded, ENTROPY_MOTION_CTU_DTYPE, n_ctu)
    d_str = codec._upload(src) if src.size else _NULL
    d_ctu, d_words, d_status = codec.alloc(32 * n_ctu), codec._upload(np.zeros(256 * n_ctu, np.uint16)), codec.alloc(max(n_ctu, 16))
    entropy_decode_motion_dev(codec, entropy_motion_params(d_ctu=d_ctu.ptr, d_words=d_words.ptr, d_coded=d_coded.ptr, d_stream=d_str.ptr, d_status=d_status.ptr,
                                                          init=table.ctypes.data if table is not None else 0, width=w, height=h, cap_words=src.size))
    return codec._fetch((d_ctu, MOTION_CTU_DTYPE, (n_ctu,)), (d_words, np.uint16, (256 * n_ctu,)), (d_status, np.uint8, (n_ctu,)))


def entropy_motion_default_init():
    """xEntropyMvDefaultInit: the default table, 7 uint16"""
    table = np.zeros(ENTROPY_MOTION_CONTEXTS, np.uint16)
    if load_library().xEntropyMvDefaultInit(table.ctypes.data) != 0:
        raise X266Error("xEntropyMvDefaultInit failed")
    return table


def entropy_encode_motion_ctu(w, h, ctu, head_mask, words, init=None, cap=ENTROPY_MOTION_MAX_BYTES):
    """xEntropyEncodeMvCtu: (the substream's first min(n_bytes, cap) bytes, n_bytes, context bins, bypass bins)"""
    src = np.ascontiguousarray(words, np.uint16).ravel()
    if src.size != 4 * bin(int(head_mask)).count("1"):
        raise X266Error("a partition is four words")
    src = np.concatenate([src, np.zeros(4, np.uint16)])                       # never an empty array: its address would be NULL
    table = _motion_table(init)
    out, bins = np.zeros(max(int(cap), 1), np.uint8), np.zeros(2, np.uint32)
    n = load_library().xEntropyEncodeMvCtu(int(w), int(h), int(ctu), int(head_mask), src.ctypes.data, table.ctypes.data if table is not None else None,
                                               out.ctypes.data if cap else None, int(cap), bins.ctypes.data)
    if n < 0:
        raise X266Error("xEntropyEncodeMvCtu: a malformed mask or a bad argument")
    return out[:min(n, int(cap))].tobytes(), n, int(bins[0]), int(bins[1])


def entropy_decode_motion_ctu(w, h, ctu, data, init=None):
    """xEntropyDecodeMvCtu: (head_mask, words uint16 [4 * parts], malformed)"""
    raw = np.frombuffer(bytes(data), np.uint8)
    table = _motion_table(init)
    mask, words, parts = np.zeros(1, np.uint64), np.zeros(256, np.uint16), np.zeros(1, np.uint32)
    rc = load_library().xEntropyDecodeMvCtu(int(w), int(h), int(ctu), raw.ctypes.data if raw.size else None, raw.size,
                                                table.ctypes.data if table is not None else None, mask.ctypes.data, words.ctypes.data, parts.ctypes.data)
    if rc < 0:
        raise X266Error("xEntropyDecodeMvCtu: a bad argument")
    return int(mask[0]), words[:4 * int(parts[0])].copy(), rc == 1


# ---- the side information (xEntropyEncodeSideGpu, xEntropyDecodeSideGpu) ------------------------------------------------------------------
SIDE_ARRAYS = (("d_kind", np.uint8), ("d_mode", np.uint8), ("d_class", np.uint8), ("d_qp", np.uint8), ("d_nnz", np.uint32))


def _side_table(init):
    if init is None:
        return None
    table = np.ascontiguousarray(init, np.uint16).ravel()
    if table.size != ENTROPY_SIDE_CONTEXTS:
        raise X266Error("init must hold %d entries" % ENTROPY_SIDE_CONTEXTS)
    return table


def entropy_side_params(**fields):
    """an x266_entropy_side_t by field name: device addresses (absent or 0: NULL) and the HOST address `init`, then n_ctu, cap_words, qp and
    chroma_qp_offset"""
    scalars = [fields.pop("n_ctu", 0), fields.pop("cap_words", 0), fields.pop("qp", 0), fields.pop("chroma_qp_offset", 0)]
    return Codec._keyword_params(EntropySideParams, "entropy_side_params", fields, scalars)


def entropy_encode_side_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyEncodeSideGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyEncodeSideGpu")


def entropy_decode_side_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyDecodeSideGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyDecodeSideGpu")


def entropy_encode_side(codec, n_ctu, kind=None, mode=None, classes=None, qps=None, nnz=None, qp=32, chroma_qp_offset=0, cap_words=None, init=None):
    """numpy convenience around xEntropyEncodeSideGpu: [6 n_ctu] entries of each array (None: NULL; init: 16 uint16 or None) -> (coded [n_ctu]
    of ENTROPY_SIDE_CTU_DTYPE, stream uint16 [cap_words], total uint64 [2]).  cap_words None: a count-only call sizes the stream exactly; words
    the call does not write are 0."""
    n_ctu = int(n_ctu)
    table = _side_table(init)
    held = {name: codec._table(a, dtype, 6 * n_ctu) for (name, dtype), a in zip(SIDE_ARRAYS, (kind, mode, classes, qps, nnz))}
    d_coded, d_tot = codec.alloc(max(32 * n_ctu, 16)), codec.alloc(16)
    p = entropy_side_params(d_coded=d_coded.ptr, d_total=d_tot.ptr, init=table.ctypes.data if table is not None else 0, n_ctu=n_ctu, qp=qp,
                            chroma_qp_offset=chroma_qp_offset, **{name: d.ptr for name, d in held.items()})
    if cap_words is None:
        entropy_encode_side_dev(codec, p)
        cap_words = codec._fetch((d_tot, np.uint64, (2,)))[0]
    cap_words = int(cap_words)
    d_str = codec._upload(np.zeros(cap_words, np.uint16)) if cap_words else _NULL
    p.d_stream, p.cap_words = d_str.ptr or None, cap_words
    entropy_encode_side_dev(codec, p)
    return codec._fetch((d_coded, ENTROPY_SIDE_CTU_DTYPE, (n_ctu,)), (d_str, np.uint16, (cap_words,)), (d_tot, np.uint64, (2,)))


def entropy_decode_side(codec, coded, stream, qp=32, chroma_qp_offset=0, init=None):
    """numpy convenience around xEntropyDecodeSideGpu: the coded records (ENTROPY_SIDE_CTU_DTYPE) and the stream's words -> (kind, mode,
    class, qp uint8 [6 n_ctu], nnz uint32 [6 n_ctu], status uint8 [n_ctu])"""
    rec = np.ascontiguousarray(coded, ENTROPY_SIDE_CTU_DTYPE).ravel()
    n_ctu = rec.size
    src = np.ascontiguousarray(stream, np.uint16).ravel()
    table = _side_table(init)
    d_coded = codec._upload(rec)
    d_str = codec._upload(src) if src.size else _NULL
    held = {name: codec.alloc(max(6 * n_ctu * np.dtype(dtype).itemsize, 16)) for name, dtype in SIDE_ARRAYS}
    d_status = codec.alloc(max(n_ctu, 16))
    entropy_decode_side_dev(codec, entropy_side_params(d_coded=d_coded.ptr, d_stream=d_str.ptr, d_status=d_status.ptr, init=table.ctypes.data if table is not None else 0,
                                                       n_ctu=n_ctu, cap_words=src.size, qp=qp, chroma_qp_offset=chroma_qp_offset,
                                                       **{name: d.ptr for name, d in held.items()}))
    return codec._fetch(*([(held[name], dtype, (6 * n_ctu,)) for name, dtype in SIDE_ARRAYS] + [(d_status, np.uint8, (n_ctu,))]))


def entropy_side_default_init():
    """xEntropySideDefaultInit: the default table, 16 uint16"""
    table = np.zeros(ENTROPY_SIDE_CONTEXTS, np.uint16)
    if load_library().xEntropySideDefaultInit(table.ctypes.data) != 0:
        raise X266Error("xEntropySideDefaultInit failed")
    return table


def entropy_encode_side_ctu(kind=None, mode=None, classes=None, qps=None, nnz=None, qp=32, chroma_qp_offset=0, init=None, cap=ENTROPY_SIDE_MAX_BYTES):
    """xEntropyEncodeSideCtu: six entries of each array (None: NULL) -> (the substream's first min(n_bytes, cap) bytes, n_bytes, context bins,
    bypass bins)"""
    held = []
    for (name, dtype), a in zip(SIDE_ARRAYS, (kind, mode, classes, qps, nnz)):
        held.append(None if a is None else np.ascontiguousarray(a, dtype).ravel())
        if held[-1] is not None and held[-1].size != 6:
            raise X266Error("%s: a CTU is six regions" % name)
    table = _side_table(init)
    out, bins = np.zeros(max(int(cap), 1), np.uint8), np.zeros(2, np.uint32)
    n = load_library().xEntropyEncodeSideCtu(*([a.ctypes.data if a is not None else None for a in held] +
                                               [int(qp), int(chroma_qp_offset), table.ctypes.data if table is not None else None, out.ctypes.data if cap else None,
                                                int(cap), bins.ctypes.data]))
    if n < 0:
        raise X266Error("xEntropyEncodeSideCtu: a bad argument")
    return out[:min(n, int(cap))].tobytes(), n, int(bins[0]), int(bins[1])


def entropy_decode_side_ctu(data, qp=32, chroma_qp_offset=0, init=None):
    """xEntropyDecodeSideCtu: (kind, mode, class, qp uint8 [6], nnz uint32 [6], malformed)"""
    raw = np.frombuffer(bytes(data), np.uint8)
    table = _side_table(init)
    got = [np.zeros(6, dtype) for _, dtype in SIDE_ARRAYS]
    rc = load_library().xEntropyDecodeSideCtu(raw.ctypes.data if raw.size else None, raw.size, int(qp), int(chroma_qp_offset),
                                              table.ctypes.data if table is not None else None, *[a.ctypes.data for a in got])
    if rc < 0:
        raise X266Error("xEntropyDecodeSideCtu: a bad argument")
    return tuple(got) + (rc == 1,)


# ---- the per-context bin statistics (xEntropyStatsLevelsGpu, xEntropyStatsSideGpu) and the tables from them ---------------------------------
def entropy_stats_rows(n_units, per_row):
    """xEntropyStatsRows: the rows of d_part for n_units regions or CTUs"""
    return int(load_library().xEntropyStatsRows(int(n_units), int(per_row)))


def entropy_stats_params(**fields):
    """an x266_entropy_stats_t by field name: device addresses (absent or 0: NULL), then n_regions"""
    scalars = [fields.pop("n_regions", 0)]
    return Codec._keyword_params(EntropyStatsParams, "entropy_stats_params", fields, scalars)


def entropy_side_stats_params(**fields):
    """an x266_entropy_side_stats_t by field name: device addresses (absent or 0: NULL), then n_ctu, qp and chroma_qp_offset"""
    scalars = [fields.pop("n_ctu", 0), fields.pop("qp", 0), fields.pop("chroma_qp_offset", 0)]
    return Codec._keyword_params(EntropySideStatsParams, "entropy_side_stats_params", fields, scalars)


def entropy_stats_levels_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyStatsLevelsGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyStatsLevelsGpu")


def entropy_stats_side_dev(codec, params, stream=0):
    codec._check(codec.L.xEntropyStatsSideGpu(codec.ctx, ctypes.byref(params) if params is not None else None, stream), "xEntropyStatsSideGpu")


def entropy_stats_levels(codec, levels, classes=None, nnz=None):
    """numpy convenience around xEntropyStatsLevelsGpu: [n_regions, 1024] int16 (and a class byte and a non-zero count per region, None:
    NULL) -> (counts uint64 [100, 2], zero bins then one bins of each context; part uint32 [rows, 100, 2], one row per
    ENTROPY_STATS_REGIONS regions)"""
    lv = np.ascontiguousarray(levels, np.int16).reshape(-1, 1024)
    n = lv.shape[0]
    rows = entropy_stats_rows(n, ENTROPY_STATS_REGIONS)
    d_level = codec._upload(lv) if n else _NULL
    d_class, d_nnz = codec._table(classes, np.uint8, n), codec._table(nnz, np.uint32, n)
    d_counts, d_part = codec.alloc(16 * ENTROPY_CONTEXTS), codec.alloc(max(8 * ENTROPY_CONTEXTS * rows, 16))
    entropy_stats_levels_dev(codec, entropy_stats_params(d_level=d_level.ptr, d_class=d_class.ptr, d_nnz=d_nnz.ptr, d_counts=d_counts.ptr, d_part=d_part.ptr,
                                                         n_regions=n))
    return codec._fetch((d_counts, np.uint64, (ENTROPY_CONTEXTS, 2)), (d_part, np.uint32, (rows, ENTROPY_CONTEXTS, 2)))


def entropy_stats_side(codec, n_ctu, kind=None, mode=None, classes=None, qps=None, nnz=None, qp=32, chroma_qp_offset=0):
    """numpy convenience around xEntropyStatsSideGpu: [6 n_ctu] entries of each array (None: NULL) -> (counts uint64 [16, 2], part uint32
    [rows, 16, 2], one row per ENTROPY_SIDE_STATS_CTUS CTUs)"""
    n_ctu = int(n_ctu)
    rows = entropy_stats_rows(n_ctu, ENTROPY_SIDE_STATS_CTUS)
    held = {name: codec._table(a, dtype, 6 * n_ctu) for (name, dtype), a in zip(SIDE_ARRAYS, (kind, mode, classes, qps, nnz))}
    d_counts, d_part = codec.alloc(16 * ENTROPY_SIDE_CONTEXTS), codec.alloc(max(8 * ENTROPY_SIDE_CONTEXTS * rows, 16))
    entropy_stats_side_dev(codec, entropy_side_stats_params(d_counts=d_counts.ptr, d_part=d_part.ptr, n_ctu=n_ctu, qp=qp, chroma_qp_offset=chroma_qp_offset,
                                                            **{name: d.ptr for name, d in held.items()}))
    return codec._fetch((d_counts, np.uint64, (ENTROPY_SIDE_CONTEXTS, 2)), (d_part, np.uint32, (rows, ENTROPY_SIDE_CONTEXTS, 2)))


def entropy_init_from_counts(counts):
    """xEntropyInitFromCounts: counts [n_contexts, 2] (zero bins, one bins; Python integers below 2^64) -> the table, n_contexts uint16"""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64).reshape(-1, 2))
    table = np.zeros(c.shape[0], np.uint16)
    if c.shape[0] and load_library().xEntropyInitFromCounts(c.ctypes.data, c.shape[0], table.ctypes.data) != 0:
        raise X266Error("xEntropyInitFromCounts: a count of 2^51 or more")
    return table


def entropy_count_region(level, cls=3, coded=True, counts=None):
    """xEntropyCountRegion: the context bins of one region ADDED to counts (uint64 [100, 2]; None: zeros), which is returned.  coded False:
    the region counts as all zero and level may be None"""
    lv = None if level is None else np.ascontiguousarray(level, np.int16).ravel()
    if lv is not None and lv.size != 1024:
        raise X266Error("a region is 1024 levels")
    out = np.zeros((ENTROPY_CONTEXTS, 2), np.uint64) if counts is None else counts
    if out.dtype != np.uint64 or out.shape != (ENTROPY_CONTEXTS, 2) or not out.flags.c_contiguous:
        raise X266Error("counts: uint64 [%d, 2]" % ENTROPY_CONTEXTS)
    if load_library().xEntropyCountRegion(lv.ctypes.data if lv is not None else None, int(cls), int(bool(coded)), out.ctypes.data) != 0:
        raise X266Error("xEntropyCountRegion: a bad argument")
    return out


def entropy_count_side_ctu(kind=None, mode=None, classes=None, qps=None, nnz=None, qp=32, chroma_qp_offset=0, counts=None):
    """xEntropyCountSideCtu: the context bins of one CTU (six entries of each array, None: NULL) ADDED to counts (uint64 [16, 2]; None:
    zeros), which is returned"""
    held = []
    for (name, dtype), a in zip(SIDE_ARRAYS, (kind, mode, classes, qps, nnz)):
        held.append(None if a is None else np.ascontiguousarray(a, dtype).ravel())
        if held[-1] is not None and held[-1].size != 6:
            raise X266Error("%s: a CTU is six regions" % name)
    out = np.zeros((ENTROPY_SIDE_CONTEXTS, 2), np.uint64) if counts is None else counts
    if out.dtype != np.uint64 or out.shape != (ENTROPY_SIDE_CONTEXTS, 2) or not out.flags.c_contiguous:
        raise X266Error("counts: uint64 [%d, 2]" % ENTROPY_SIDE_CONTEXTS)
    if load_library().xEntropyCountSideCtu(*([a.ctypes.data if a is not None else None for a in held] + [int(qp), int(chroma_qp_offset), out.ctypes.data])) != 0:
        raise X266Error("xEntropyCountSideCtu: a bad argument")
    return out
