"""GPU: the HIP path against the REAL reference, directly and in volume (missing #3).

Every other -m gpu test compares with the oracle (this repo's restatement, itself pinned to the reference): valid, but one hop
longer than needed.  Here the batch kernels' outputs are compared with the answers of the reference's own partialButterfly32 x 2
(src_tb/dct32.c:197-198) on 1.2e5 mixed blocks, of its satd8x8 (src_tb/satd.c:31-118) on 1.3e6 blocks, and of partialButterfly32
itself for the 1-D pass at the two shifts dct32_genNew uses (src_tb/dct32.c:180-181).  Those answers were recorded where the
reference lies (tests/golden/gen_ref_digests.py): tests/golden/ref_digests.json holds the SHA-256 of each output array."""
import numpy as np
import pytest

from _util import dct_edge_blocks, digest, extremes_np, fullrange_np, ref_digest, residual_np, satd_edge_blocks

pytestmark = pytest.mark.gpu


def _mixed(n_tri, n_full, n_ext, unit, seed, edge):
    parts = [residual_np(n_tri * unit, seed).reshape(n_tri, unit), fullrange_np(n_full * unit, seed + 0x1000).reshape(n_full, unit),
             extremes_np(n_ext * unit, seed + 0x2000).reshape(n_ext, unit), edge]
    x = np.concatenate(parts).astype(np.int16)
    return x[np.random.RandomState(seed).permutation(x.shape[0])]          # the kinds interleaved, not in runs


def _where(got, want):
    """the message of a digest mismatch: which blocks leave the oracle (pinned to the same digests by tests/test_oracle_vs_ref.py)"""
    bad = np.flatnonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))
    return "differs from the reference's digest; %d block(s) differ from the oracle, the first: %s" % (bad.size, bad[:1].tolist())


def test_dct32_forward_batch_equals_the_reference_on_120k_mixed_blocks(codec, oracle):
    x = _mixed(80000, 30000, 10000, 1024, 0x51, dct_edge_blocks()[0])
    assert x.shape[0] >= 100000
    got = codec.dct32_fwd(x)                                              # host-pointer call: staging pipeline + the batch kernel
    assert digest(got) == ref_digest("gpu_vs_reference.dct32_fwd"), _where(got, oracle.dct32_fwd(x, threads=8))


def test_satd8x8_batch_equals_the_reference_on_1m3_mixed_blocks(codec, oracle):
    x = _mixed(900000, 300000, 100000, 64, 0x52, satd_edge_blocks()[0])
    assert x.shape[0] >= 1000000
    want = ref_digest("gpu_vs_reference.satd8x8")
    for variant in (0, 1, 3):                                             # by batch size / staged kernel / LDS-DMA kernel
        codec.set_option("satd_variant", variant)
        got = codec.satd8x8(x)
        assert digest(got) == want, (variant, _where(got, oracle.satd8x8(x, threads=8)))
    codec.set_option("satd_variant", 0)


@pytest.mark.parametrize("shift", [4, 11])
def test_one_dimensional_pass_equals_partialButterfly32(codec, oracle, shift):
    """xDct32PassDev = partialButterfly32(src, dst, shift, 32) with its transposed store, 1000 mixed blocks per shift"""
    x = _mixed(600, 300, 84, 1024, 0x53 + shift, dct_edge_blocks()[0])[:1000]
    got = codec.dct32_pass(x, shift)
    assert digest(got) == ref_digest("gpu_vs_reference.dct32_pass_%d" % shift), _where(got, np.stack([oracle.dct32_pass(b, shift) for b in x]))


def test_fused_forward_half_equals_the_reference(codec, oracle):
    """the coefficients xDct32FwdInvBatchDev writes are the reference's (its inverse half has no upstream counterpart)"""
    x = _mixed(6000, 1500, 500, 1024, 0x54, dct_edge_blocks()[0])
    n = x.shape[0]
    d_in, d_coef, d_rec = codec.alloc(x.nbytes), codec.alloc(x.nbytes), codec.alloc(x.nbytes)
    d_in.upload(x)
    codec.dct32_fwd_inv_dev(d_in.ptr, d_coef.ptr, d_rec.ptr, n)
    codec.stream_sync()
    got = d_coef.download(np.int16, n * 1024).reshape(n, 1024)
    assert digest(got) == ref_digest("gpu_vs_reference.fused_forward"), _where(got, oracle.dct32_fwd(x, threads=8))
