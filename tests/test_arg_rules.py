"""CPU: the argument rules of the device entry points (x266_amd/csrc/x266_args.hpp: NULL, alignment, "the span fits in the address
space", "no output overlaps another buffer", sizes and scalar ranges) against the contract as tests/cpp/arg_rules_check.cpp writes
it down: one row per entry point, one walk of single perturbations of a base tuple, with made-up addresses.  The driver is a
stand-alone program, built twice -- plain, and with the address and undefined-behaviour sanitizers.  Its rows must be the header's
device entry points, found by the form of their declarations, and its per-entry-point alignment lines the ones include/x266hip.h
states in front of each (and, for the ...Dev calls, tests/test_gpu_placement.py places buffers at).  g++ only: no GPU, no HIP.
The surface tests need the built library and no GPU: every entry point is exported and refuses a NULL context."""
import ctypes
import os
import re
import subprocess

import numpy as np

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@_cpp_driver.needs_gxx
def test_the_rules_hold_and_state_the_headers_alignments(tmp_path):
    exe, r = _cpp_driver.build(tmp_path, "arg_rules_check")
    assert r.returncode == 0, r.stderr[-4000:]
    text = _cpp_driver.run(exe)
    lines = dict(re.findall(r"^(x\w+): (.*)$", text, re.M))
    got = {name: {k: int(v) for k, v in (i.split() for i in items.split(", "))} for name, items in lines.items()}
    from test_gpu_placement import device_entry_points, header_alignments
    declared = device_entry_points()
    assert len(declared) >= 60, sorted(declared)                            # a parser that finds too few must not pass quietly
    assert set(got) == set(declared), sorted(set(got) ^ set(declared))       # a new entry point needs its row in the driver
    assert "%d entry points" % len(declared) in text
    stated = header_alignments(every=True)
    for name, ptrs in declared.items():
        assert got[name] == stated.get(name), (name, got[name], stated.get(name))   # the line in front of the declaration
        assert sorted(stated[name]) == sorted(ptrs), (name, sorted(stated[name]), sorted(ptrs))   # ... names its device pointers, all of them
    placed = header_alignments()
    assert len(placed) >= 37
    assert {n: a for n, a in got.items() if n.endswith("Dev")} == placed
    assert "Frames are 16-byte aligned, d_stats 4, d_total 8, d_luma and d_chroma 4, the byte arrays (d_class, d_mask, d_ctrl) 1" in open(
        os.path.join(ROOT, "include", "x266hip.h")).read()


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, "arg_rules_check")


def test_the_library_exports_every_entry_point_and_a_null_context_is_refused():
    import x266_amd
    from test_gpu_placement import device_entry_points
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    names = sorted(device_entry_points())
    assert len(names) >= 60
    for name in names:
        assert name in exported and hasattr(lib, name), name
        fn = getattr(lib, name)
        null = [None if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else 0 for t in fn.argtypes]
        assert fn(*null) < 0, name                                            # a NULL context is refused, not dereferenced


def test_codec_has_the_bi_directional_methods_and_the_weights_layout():
    import x266_amd
    for method in ("motion_comp_bi_qpel", "satd8x8_bi_costs", "satd8x8_refine_bi_qpel"):
        assert callable(getattr(x266_amd.Codec, method)) and callable(getattr(x266_amd.Codec, method + "_dev")), method
    wp = x266_amd.Codec.wp_params(w=((2, 3, 4), (5, 6, 7)), o=((-1, -2, -3), (1, 2, 3)), log2_denom=(1, 7))
    raw = bytes(wp)
    assert len(raw) == 26 and raw[24:] == bytes([1, 7])                     # int16 w[2][3], int16 o[2][3], uint8 log2_denom[2]
    assert np.frombuffer(raw[:24], np.int16).tolist() == [2, 3, 4, 5, 6, 7, -1, -2, -3, 1, 2, 3]
