"""The compact motion stream (include/x266hip.h: xMotionPackGpu, xMotionUnpackGpu, xMotionReconstructGpu): the numpy calls around
Codec.motion_pack_dev, Codec.motion_unpack_dev and Codec.motion_reconstruct_dev, built from the pieces the Codec's own numpy methods are built from, and the three host helpers of the library
(xMotionWalk, xMotionPredictor, xMotionVectorBits).  No arithmetic lives here."""
import ctypes

import numpy as np

from ._lib import MOTION_CTU_DTYPE, Codec, MotionParams, X266Error, _NULL, load_library


def motion_params(**fields):
    """an x266_motion_t by field name: device addresses (absent or 0: NULL), then width, height and cap_words"""
    scalars = [fields.pop("width", 0), fields.pop("height", 0), fields.pop("cap_words", 0)]
    return Codec._keyword_params(MotionParams, "motion_params", fields, scalars)


def motion_pack(codec, mv, level, w, h, cap_words=None):
    """numpy convenience around xMotionPackGpu: the field [nb, 2] int16 and the level bytes [nb] of a w x h frame -> (records [n_ctu] of
    MOTION_CTU_DTYPE, stream uint16 [cap_words], total uint64 [2]).  cap_words None: a count-only call sizes the stream exactly; words the
    call does not write are 0."""
    nb, n_ctu = (w // 8) * (h // 8), codec.ctu_count(w, h)
    d_mv, d_level = codec._upload(codec._records(mv, nb)), codec._table(level, np.uint8, nb)
    d_ctu, d_tot = codec.alloc(32 * n_ctu), codec.alloc(16)
    p = motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_total=d_tot.ptr, width=w, height=h)
    if cap_words is None:
        codec.motion_pack_dev(p)
        cap_words = codec._fetch((d_tot, np.uint64, (2,)))[0]
    cap_words = int(cap_words)
    d_str = codec._upload(np.zeros(cap_words, np.uint16)) if cap_words else _NULL
    p.d_stream, p.cap_words = d_str.ptr or None, cap_words
    codec.motion_pack_dev(p)
    return codec._fetch((d_ctu, MOTION_CTU_DTYPE, (n_ctu,)), (d_str, np.uint16, (cap_words,)), (d_tot, np.uint64, (2,)))


def motion_unpack(codec, records, stream, w, h):
    """numpy convenience around xMotionUnpackGpu: records (MOTION_CTU_DTYPE) and the stream's words of a w x h frame -> (mv [nb, 2] int16,
    cost [nb] uint32 -- all 0 --, level [nb] uint8)"""
    nb, n_ctu = (w // 8) * (h // 8), codec.ctu_count(w, h)
    words = np.ascontiguousarray(stream, np.uint16).ravel()
    d_ctu = codec._table(records, MOTION_CTU_DTYPE, n_ctu)
    d_str = codec._upload(words) if words.size else _NULL
    d_mv, d_level = codec.alloc(8 * nb), codec.alloc(max(nb, 16))
    codec.motion_unpack_dev(motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_str.ptr, width=w, height=h, cap_words=words.size))
    raw, level = codec._fetch((d_mv, np.uint8, (nb * 8,)), (d_level, np.uint8, (nb,)))
    return raw.view(np.int16).reshape(nb, 4)[:, :2].copy(), raw.view(np.uint32).reshape(nb, 2)[:, 1].copy(), level


# ---- the host helpers: the library's own functions, no device ------------------------------------------------------------------------------
def motion_walk(w, h, ctu, head_mask):
    """xMotionWalk: (heads, levels) of the partitions of CTU `ctu` under head_mask in coding order, uint8 arrays of length parts"""
    head, level = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    parts = load_library().xMotionWalk(int(w), int(h), int(ctu), int(head_mask), head.ctypes.data, level.ctypes.data)
    if parts < 0:
        raise X266Error("xMotionWalk: a malformed mask or a bad argument")
    return head[:parts], level[:parts]


def motion_predictor(w, h, field, X, Y, level):
    """xMotionPredictor: the causal predictor (px, py) of the whole node of `level` at block (X, Y); field = the vectors [nb, 2] int16"""
    rec = np.ascontiguousarray(Codec._records(field, (w // 8) * (h // 8)))
    p = (ctypes.c_int16 * 2)()
    if load_library().xMotionPredictor(int(w), int(h), rec.ctypes.data, int(X), int(Y), int(level), ctypes.addressof(p)) != 0:
        raise X266Error("xMotionPredictor: a bad argument")
    return int(p[0]), int(p[1])


def motion_vector_bits(d):
    """xMotionVectorBits: L(d), or -1 beyond |d| = 65535"""
    return int(load_library().xMotionVectorBits(int(d)))


def motion_reconstruct(codec, records, stream, w, h):
    """numpy convenience around xMotionReconstructGpu: records (MOTION_CTU_DTYPE) and the stream's words of a w x h frame, of which only the
    differences (words 2 and 3 of a partition) are read -> (mv [nb, 2] int16, cost [nb] uint32 -- all 0 --, level [nb] uint8)"""
    nb, n_ctu = (w // 8) * (h // 8), codec.ctu_count(w, h)
    words = np.ascontiguousarray(stream, np.uint16).ravel()
    d_ctu = codec._table(records, MOTION_CTU_DTYPE, n_ctu)
    d_str = codec._upload(words) if words.size else _NULL
    d_mv, d_level = codec.alloc(8 * nb), codec.alloc(max(nb, 16))
    codec.motion_reconstruct_dev(motion_params(d_mv=d_mv.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr, d_stream=d_str.ptr, width=w, height=h, cap_words=words.size))
    raw, level = codec._fetch((d_mv, np.uint8, (nb * 8,)), (d_level, np.uint8, (nb,)))
    return raw.view(np.int16).reshape(nb, 4)[:, :2].copy(), raw.view(np.uint32).reshape(nb, 2)[:, 1].copy(), level
