"""CPU: the quantiser's definition (tests/_quant_ref.py, the statement the GPU tests compare with) has the properties the header
states, and the new entry points exist and refuse to run without a device.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _quant_ref as Q
import x266_amd
from _util import ROOT


def test_constants_are_reciprocal():
    """f[r] * g[r] = 2^20 up to rounding of f: catches a mistyped constant"""
    for r in range(6):
        assert abs(int(Q.F[r]) * int(Q.G[r]) - (1 << 20)) <= 64, r


@pytest.mark.parametrize("sign", [1, -1])
def test_worked_value(sign):
    assert int(Q.quant(sign * 1000, 5, 22, 171)) == sign * 31
    assert int(Q.dequant(sign * 31, 5, 22)) == sign * 992


def test_bounds_at_the_extreme_inputs():
    """|level| <= 13108 (no forward clip), and both products stay below 2^30 (int32 exact, 24-bit multiply-add operands below 2^16)"""
    seen = 0
    for n in (2, 3, 4, 5):
        for qp in (0, 51):
            assert Q.qbits(n, qp) >= 16
            assert int(Q.G[qp % 6] << (qp // 6)) < 1 << 16 and int(Q.F[qp % 6]) < 1 << 16
            for rounding in (0, 511):
                lv, pre = Q.quant_unsigned(32768, n, qp, rounding)
                assert 0 <= int(pre) < 1 << 30
                assert int(lv) <= 13108
                seen = max(seen, int(lv))
            for level in (13108, -13108, 32767, -32768):
                _, prod = Q.dequant_unclipped(level, n, qp)
                assert abs(int(prod)) < 1 << 30
    assert seen == 13107                                                   # 32768 * 26214 = 13107 * 2^16 exactly, and the rounding adds less than 1
    assert int(Q.quant(-32768, 5, 0, 511)) == -13107


def test_dequantiser_needs_its_clip():
    assert int(Q.dequant_unclipped(13107, 5, 0)[0]) == 32768
    assert int(Q.dequant(13107, 5, 0)) == 32767
    assert int(Q.dequant(-32768, 2, 51)) == -32768


def test_six_qp_steps_halve_the_level():
    c = np.arange(-32768, 32768, 7, dtype=np.int64)
    for n in (2, 3, 4, 5):
        for qp in (0, 5, 22, 45):
            a, b = np.abs(Q.quant(c, n, qp, 0)), np.abs(Q.quant(c, n, qp + 6, 0))
            assert np.array_equal(b, a >> 1), (n, qp)


def test_regions_statement_counts_and_clamps():
    x = np.zeros((3, 1024), np.int16)
    x[1, 5], x[2, :] = 1000, -32768
    lv, nnz = Q.quant_regions(x, False, np.array([3, 3, 0], np.uint8), np.array([22, 22, 63], np.uint8), 0, 171)
    assert nnz.tolist() == [0, 1, 1024] and lv[1, 5] == 31
    assert np.array_equal(lv[2], Q.quant(x[2], 2, 51, 171))              # byte 63 -> qp 51, class 0 -> n = 2


def test_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    for name in ("xQuantRegionsGpu", "xDct32CodeCtuTilesGpu"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert "as recalled, unverified offline" in hdr[hdr.index("Quantisation"):hdr.index("int xQuantRegionsGpu(")]
    x266_amd.build_library()
    lib = x266_amd.load_library()
    assert len(lib.xQuantRegionsGpu.argtypes) == 11 and len(lib.xDct32CodeCtuTilesGpu.argtypes) == 12
    # a NULL context is rejected, not dereferenced
    assert lib.xQuantRegionsGpu(None, 0, None, None, 4, None, None, 22, 171, None, None) < 0
    assert lib.xDct32CodeCtuTilesGpu(None, None, None, 64, 64, None, 22, 171, None, None, None, None) < 0
    for name in ("quant_regions_dev", "dct32_code_ctu_tiles_dev", "quant_regions", "code_ctu_tiles"):
        assert callable(getattr(x266_amd.Codec, name)), name


def test_binding_refuses_without_a_device():
    """there is no CPU path: without a device no context exists, and the conveniences raise instead of computing"""
    lib = x266_amd.load_library()
    if lib.xHipDeviceCount() > 0:
        pytest.skip("a device is present: the calls run in tests/test_gpu_quant.py")
    with pytest.raises(x266_amd.X266Error):
        x266_amd.Codec(0).quant_regions(np.zeros((1, 1024), np.int16), qp=22)
    ctx = ctypes.c_void_p()
    assert lib.xHipCodecInit(ctypes.byref(ctx), 0) < 0 and not ctx.value
