"""CPU: the surface of the seeded search, xSatd8x8SeededSearchGpu: header, struct layout, bindings, and that the kernel and the rules
share one copy of the arithmetic.  The call keeps its device pointers in a host-read struct; tests/cpp/struct_rules_check.cpp holds its
argument rules (x266_amd/csrc/x266_args.hpp: seeded_search) at both seed scales and tests/test_struct_arg_rules.py runs it.  No GPU, no
HIP."""
import ctypes
import os
import re
import subprocess

import pytest

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "xSatd8x8SeededSearchGpu"
ALIGN = {"d_cur": 16, "d_ref": 16, "d_seed": 8, "d_best": 8, "d_j": 4}
FIELDS = ["d_cur", "d_ref", "d_seed", "d_best", "d_j", "width", "height", "seed_scale", "centres", "range", "lambda_q4"]


@_cpp_driver.needs_gxx
def test_the_header_declares_the_call_outside_the_one_table():
    """context first, stream last, the device pointers in the struct: the parser of the one table must not count it, and the struct's
    field comments state the alignments the driver holds"""
    from test_gpu_placement import device_entry_points, header_alignments
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    assert "hierarchical motion search: a seeded SATD search around per-block starting vectors" in hdr
    assert CALL not in device_entry_points() and CALL not in header_alignments(every=True)
    assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_seed_t \*p, void \*stream\);" % CALL, hdr)
    body = re.search(r"typedef struct x266_seed_t \{(.*?)\} x266_seed_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == FIELDS
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s*(d_\w+);[^\n]*?(\d+)-byte aligned", body)}
    assert stated == ALIGN, stated
    assert re.search(r"\*\s*d_j;[^\n]*or NULL", body)
    for field in ("d_cur", "d_ref", "d_seed", "d_best"):
        assert not re.search(r"\*\s*%s;[^\n]*NULL" % field, body), field
    _cpp_driver.assert_driver_follows_header("x266_seed_t", (CALL,), outputs_marked=True)
    for consequence in ("at range 8", "entry [49 b + 24]"):                   # the two consequences the GPU tests rely on
        assert consequence in hdr, consequence


def test_the_kernel_and_the_rules_share_one_copy_of_the_arithmetic():
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, rules, shared = (open(os.path.join(csrc, n)).read() for n in ("seeded_search_kernels.hip", "x266_args.hpp", "x266_seed.hpp"))
    assert '#include "x266_seed.hpp"' in kernel and '#include "x266_seed.hpp"' in rules
    for name in ("seed_clamp", "seed_centre_list", "seed_walk_step", "seed_code_length", "seed_vector_cost", "kSeedMaxRange", "kSeedCentreBits"):
        assert re.search(r"\b%s\b" % name, shared), name
    for name in ("seed_centre_list", "seed_walk_step", "seed_vector_cost"):
        assert name in kernel, name
    for name in ("kSeedMaxRange", "kSeedCentreBits", "seed_cells"):
        assert name in rules, name
    assert "8183" not in kernel and "8183" not in rules                        # the clamp is stated once
    # the search's per-wave pieces are used, not copied
    blocks, me = open(os.path.join(csrc, "x266_me_blocks.hpp")).read(), open(os.path.join(csrc, "me_search.hip")).read()
    for name in ("make_lane_ops", "hadamard_lane", "load_window8", "tiled_ref_dword", "sad16"):
        assert len(re.findall(r"__device__ __forceinline__ [^\n]*\b%s\(" % name, blocks)) == 1, name
        assert not re.search(r"__device__ __forceinline__ [^\n]*\b%s\(" % name, me + kernel), name
        assert name in me and name in kernel, name


def test_the_library_exports_the_call_and_it_refuses_null():
    import x266_amd
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert CALL in exported and hasattr(lib, CALL)
    fn = getattr(lib, CALL)
    assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.SeedParams)
    p = x266_amd.Codec.seed_params(width=96, height=80, seed_scale=1, centres=31, range=2, lambda_q4=16, d_seed=4096)
    assert ctypes.sizeof(x266_amd.SeedParams) == 64
    assert (p.width, p.height, p.seed_scale, p.centres, p.range, p.lambda_q4) == (96, 80, 1, 31, 2, 16)
    assert not p.d_cur and p.d_seed == 4096 and not p.d_j
    assert [f[0] for f in x266_amd.SeedParams._fields_] == FIELDS
    with pytest.raises(TypeError):
        x266_amd.Codec.seed_params(d_nothing=1)
    assert fn(None, ctypes.byref(p), None) == -1                              # a NULL context is refused, not dereferenced
    assert fn(None, None, None) == -1                                         # ... and so is a NULL p
    for method in ("seed_params", "satd_seeded_search_dev", "seeded_search_tiles"):
        assert callable(getattr(x266_amd.Codec, method)), method
