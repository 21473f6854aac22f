"""CPU: the oracle against the real reference's answers on seeded inputs, recorded where the reference lies
(tests/golden/gen_ref_digests.py -> tests/golden/ref_digests.json: SHA-256 of each output array); the committed
golden vectors (test_oracle_golden.py) carry the same pin block by block."""
import numpy as np

from _util import digest, extremes_np, fullrange_np, ref_digest, residual_np


def _mixed(n_each, unit, seed):
    return np.concatenate([
        residual_np(n_each * unit, seed).reshape(n_each, unit),
        fullrange_np(n_each * unit, seed + 1).reshape(n_each, unit),
        extremes_np(n_each * unit, seed + 2).reshape(n_each, unit)])


def test_table_identical(oracle):
    assert digest(oracle.table()) == ref_digest("oracle_vs_ref.table")


def test_dct32_fwd_identical(oracle):
    x = _mixed(3000, 1024, 11)
    assert digest(oracle.dct32_fwd(x, threads=4)) == ref_digest("oracle_vs_ref.dct32_fwd")


def test_dct32_single_pass_identical(oracle):
    x = _mixed(40, 1024, 21)
    got = np.stack([oracle.dct32_pass(blk, shift) for blk in x for shift in (4, 11)])
    assert digest(got) == ref_digest("oracle_vs_ref.dct32_pass")


def test_satd_identical(oracle):
    d = _mixed(100000, 64, 31)
    assert digest(oracle.satd8x8(d, threads=4)) == ref_digest("oracle_vs_ref.satd8x8")
