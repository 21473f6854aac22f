"""The inter partition decision (include/x266hip.h: xInterPartitionDecideGpu): the numpy calls around Codec.inter_partition_decide_dev,
built from the pieces the Codec's own numpy methods are built from.  No arithmetic lives here."""
import numpy as np

from ._lib import PART_CTU_DTYPE, Codec, PartParams


def part_params(**fields):
    """an x266_part_t by field name: device addresses (absent or 0: NULL), then width, height, range and lambda_q4"""
    scalars = [fields.pop("width", 0), fields.pop("height", 0), fields.pop("range", 0), fields.pop("lambda_q4", 0)]
    return Codec._keyword_params(PartParams, "part_params", fields, scalars)


def node_count(w, h):
    """the whole nodes of levels 1..3 of a w x h frame: the records of d_nodes"""
    return sum(((w // 8) >> k) * ((h // 8) >> k) for k in (1, 2, 3))


def partition_decide(codec, cur_tiles, ref_tiles, w, h, mv, rng=0, lambda_q4=0, want_nodes=False):
    """numpy convenience around xInterPartitionDecideGpu: two tile arrays of a w x h frame (uint8, 512 bytes per tile) and the quarter-sample
    field [nb, 2] int16 -> (mv [nb, 2] int16, satd [nb] uint32, level [nb] uint8, records [n_ctu] of PART_CTU_DTYPE, and with want_nodes
    the whole nodes' (mv [n, 2] int16, jw [n] uint32), else None)"""
    nb, n_ctu, nn = (w // 8) * (h // 8), codec.ctu_count(w, h), node_count(w, h)
    d_cur, d_ref, d_mv = codec._frame(cur_tiles, w, h), codec._frame(ref_tiles, w, h), codec._upload(codec._records(mv, nb))
    d_out, d_level, d_ctu = codec.alloc(8 * nb), codec.alloc(max(nb, 16)), codec.alloc(16 * n_ctu)
    d_nodes = codec.alloc(max(8 * nn, 16)) if want_nodes else None
    codec.inter_partition_decide_dev(part_params(d_cur=d_cur.ptr, d_ref=d_ref.ptr, d_mv=d_mv.ptr, d_out=d_out.ptr, d_level=d_level.ptr, d_ctu=d_ctu.ptr,
                                                 d_nodes=d_nodes.ptr if want_nodes else 0, width=w, height=h, range=rng, lambda_q4=lambda_q4))
    raw, level, ctu = codec._fetch((d_out, np.uint8, (nb * 8,)), (d_level, np.uint8, (nb,)), (d_ctu, PART_CTU_DTYPE, (n_ctu,)))
    nodes = None
    if want_nodes:
        n = codec._fetch((d_nodes, np.uint8, (nn * 8,)))
        nodes = (n.view(np.int16).reshape(nn, 4)[:, :2].copy(), n.view(np.uint32).reshape(nn, 2)[:, 1].copy())
    return raw.view(np.int16).reshape(nb, 4)[:, :2].copy(), raw.view(np.uint32).reshape(nb, 2)[:, 1].copy(), level, ctu, nodes
