"""CPU: the surface of xRdoQuantRegionsGpu and xLevelsBitsGpu: header, struct layout, exports, bindings, and that the rate tables stand
in one file only.  The two calls keep their device pointers in a host-read struct; tests/cpp/struct_rules_check.cpp holds their argument
rules (x266_amd/csrc/x266_args.hpp: rdoq_regions, levels_bits) and tests/test_struct_arg_rules.py runs it.  No GPU, no HIP."""
import ctypes
import glob
import os
import re
import subprocess

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xRdoQuantRegionsGpu", "xLevelsBitsGpu")
HELPERS = ("xLevelBits", "xLastPosBits", "xCgFlagBits")


@_cpp_driver.needs_gxx
def test_the_header_declares_the_two_calls_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count them, and the
    struct's field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    for name in CALLS:
        assert name not in declared and name not in header_alignments(every=True), name
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_rdoq_t \*p, void \*stream\);" % name, hdr), name
    body = re.search(r"typedef struct x266_rdoq_t \{(.*?)\} x266_rdoq_t;", hdr, re.S).group(1)
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == {"d_coef": 16, "d_level": 16, "d_nnz": 4, "d_stat": 8}, stated
    for field in ("d_class", "d_qp"):
        assert re.search(r"\*\s*%s;[^\n]*any alignment" % field, body)
    assert "rdoq: may be NULL; bits: required" in body                        # d_stat, the one field whose comment does not say "or NULL"
    _cpp_driver.assert_driver_follows_header("x266_rdoq_t", CALLS, may_be_null={("xRdoQuantRegionsGpu", "d_stat")})
    for name in HELPERS:
        assert re.search(r"int\s+%s\(" % name, hdr), name


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + HELPERS:
        assert name in exported and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                   # bound with argument types
    p = x266_amd.Codec.rdoq_params(n_regions=3, qp=30, lam=368)
    assert ctypes.sizeof(x266_amd.RdoqParams) == 64 and p.n_regions == 3 and p.qp == 30 and p.lambda_ == 368 and not p.d_level
    assert x266_amd.RDOQ_REGION_DTYPE.itemsize == 16
    for name in CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes[1] is ctypes.POINTER(x266_amd.RdoqParams)
        assert fn(None, ctypes.byref(p), None) == -1, name                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1, name                                # ... and so is a NULL p
    for method in ("rdoq_params", "rdo_quant", "rdo_quant_dev", "levels_bits", "levels_bits_dev", "level_bits", "last_pos_bits", "cg_flag_bits"):
        assert callable(getattr(x266_amd.Codec, method)), method


def test_the_rate_tables_stand_in_one_file():
    """x266_rdoq.hpp holds the one copy: the tables' values appear there, and no other file under csrc/ defines a rate function or
    spells the significance table out again; the kernels and the ABI reach them through the header's functions"""
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    home = open(os.path.join(csrc, "x266_rdoq.hpp")).read()
    for pair in ("10u : 24u", "22u : 12u", "36u : 6u", "24u : 10u", "22u : 11u", "26u : 9u"):     # sig[0..2], gt1, gt2, cgf as (1 : 0)
        assert pair in home, pair
    functions = ("rdoq_sig_bits", "rdoq_gt1_bits", "rdoq_gt2_bits", "rdoq_cg_flag_bits", "rdoq_rem", "rdoq_level_bits", "rdoq_last_pos", "rdoq_err",
                 "rdoq_choose")
    for name in functions:
        assert len(re.findall(r"\b(?:unsigned|uint64_t|RdoqChoice)\s+%s\(" % name, home)) == 1, name
    table = re.compile(r"\{\s*24\s*,\s*10\s*\}|\{\s*12\s*,\s*22\s*\}|\{\s*6\s*,\s*36\s*\}|\{\s*9\s*,\s*26\s*\}")
    for path in sorted(glob.glob(os.path.join(csrc, "*.h*")) + glob.glob(os.path.join(csrc, "*.cpp"))):
        if os.path.basename(path) == "x266_rdoq.hpp":
            continue
        text = open(path).read()
        for name in functions:
            assert not re.search(r"\b(?:unsigned|uint64_t|int|RdoqChoice)\s+%s\(" % name, text), (path, name)
        assert not table.search(text), path
        for pair in ("10u : 24u", "22u : 12u", "36u : 6u"):
            assert pair not in text, (path, pair)
    # ... and x266_rdoq.hpp restates neither the quantiser's constants nor the scan
    for foreign in ("26214", "23302", "20560", "18396", "14564", "level_diag"):
        assert foreign not in home, foreign
    users = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*.hip"))) if "x266_rdoq.hpp" in open(p).read()]
    assert users == ["rdoq_kernels.hip", "x266hip_abi.hip"], users
