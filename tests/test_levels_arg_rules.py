"""CPU: the surface of xLevelsPackGpu and xLevelsUnpackGpu: header, struct layout, exports, bindings.  The two calls keep their device
pointers in a host-read struct; tests/cpp/struct_rules_check.cpp holds their argument rules (x266_amd/csrc/x266_args.hpp: levels_pack,
levels_unpack) and tests/test_struct_arg_rules.py runs it.  No GPU, no HIP."""
import ctypes
import os
import re
import subprocess

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xLevelsPackGpu", "xLevelsUnpackGpu")


@_cpp_driver.needs_gxx
def test_the_header_declares_the_two_calls_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count them, and the
    struct's field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    for name in CALLS:
        assert name not in declared and name not in header_alignments(every=True), name
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_levels_t \*p, void \*stream\);" % name, hdr), name
    body = re.search(r"typedef struct x266_levels_t \{(.*?)\} x266_levels_t;", hdr, re.S).group(1)
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == {"d_level": 16, "d_nnz": 4, "d_region": 8, "d_stream": 16, "d_total": 8}, stated
    assert re.search(r"\*\s*d_class;[^\n]*any alignment", body)
    _cpp_driver.assert_driver_follows_header("x266_levels_t", CALLS)


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + ("xLevelScan", "xLevelsScanChunk"):
        assert name in exported and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                   # bound with argument types
    p = x266_amd.Codec.levels_params(n_regions=3, cap_words=5)
    assert ctypes.sizeof(x266_amd.LevelsParams) == 64 and p.n_regions == 3 and p.cap_words == 5 and not p.d_level
    assert x266_amd.LEVEL_REGION_DTYPE.itemsize == 32
    for name in CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes[1] is ctypes.POINTER(x266_amd.LevelsParams)
        assert fn(None, ctypes.byref(p), None) == -1, name                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1, name                                # ... and so is a NULL p
    assert lib.xLevelScan(4, None) == -1
    for method in ("levels_pack", "levels_unpack", "levels_pack_dev", "levels_unpack_dev", "levels_params", "level_scan"):
        assert callable(getattr(x266_amd.Codec, method)), method
