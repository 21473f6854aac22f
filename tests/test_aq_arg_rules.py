"""CPU: the surface of xAqStatsGpu, xAqDecideGpu and xWeightsFromTotals: header, struct layout, exports, bindings.  The two device calls
keep their pointers in a host-read struct; tests/cpp/struct_rules_check.cpp holds their argument rules (x266_amd/csrc/x266_args.hpp:
aq_stats, aq_decide, weights_from_totals) and tests/test_struct_arg_rules.py runs it.  No GPU, no HIP."""
import ctypes
import os
import re
import subprocess

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xAqStatsGpu", "xAqDecideGpu")


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count them, and the
    struct's field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    for name in CALLS:
        assert name not in declared and name not in header_alignments(every=True), name
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_aq_t \*p, void \*stream\);" % name, hdr), name
    assert re.search(r"int xAqTotalsChunk\(void\);", hdr)
    assert re.search(r"int xWeightsFromTotals\(const int64_t cur\[8\], const int64_t ref\[8\], int list, x266_wp_t \*wp\);", hdr)
    body = re.search(r"typedef struct x266_aq_t \{(.*?)\} x266_aq_t;", hdr, re.S).group(1)
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == {"d_src": 16, "d_tile": 16, "d_total": 8, "d_offset": 2}, stated
    assert re.search(r"\*\s*d_qp;[^\n]*any alignment", body)
    _cpp_driver.assert_driver_follows_header("x266_aq_t", CALLS)
    rec = re.search(r"typedef struct x266_aq_tile_t \{(.*?)\} x266_aq_tile_t;", hdr, re.S).group(1)
    assert re.findall(r"\b([a-z0-9_]+)[,;]", rec) == ["sum_y", "ssq_y", "sum_u", "ssq_u", "sum_v", "ssq_v", "energy", "log2_q8"]


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + ("xAqTotalsChunk", "xWeightsFromTotals"):
        assert name in exported and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                   # bound with argument types
    p = x266_amd.Codec.aq_params(width=48, height=80, mode=2, strength_q8=300, qp=31, chroma_qp_offset=-3)
    assert ctypes.sizeof(x266_amd.AqParams) == 64 and (p.width, p.height, p.mode, p.strength_q8, p.qp, p.chroma_qp_offset) == (48, 80, 2, 300, 31, -3)
    assert not p.d_src and not p.d_qp
    assert [f[0] for f in x266_amd.AqParams._fields_[:5]] == ["d_src", "d_tile", "d_total", "d_offset", "d_qp"]
    assert x266_amd.AQ_TILE_DTYPE.itemsize == 32 and x266_amd.AQ_TILE_DTYPE.names[6:] == ("energy", "log2_q8")
    for name in CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes[1] is ctypes.POINTER(x266_amd.AqParams)
        assert fn(None, ctypes.byref(p), None) == -1, name                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1, name                                # ... and so is a NULL p
    chunk = lib.xAqTotalsChunk()
    assert chunk >= 64 and chunk % 64 == 0 and chunk == x266_amd.aq_totals_chunk()
    assert lib.xWeightsFromTotals(None, None, 0, None) == -1
    for method in ("aq_params", "aq_stats", "aq_decide", "aq_stats_dev", "aq_decide_dev", "weights_from_totals"):
        assert callable(getattr(x266_amd.Codec, method)), method
