"""CPU: the surface and the argument rules of xEntropyStatsLevelsGpu and xEntropyStatsSideGpu: header, struct layouts, exports, bindings,
and the rule functions of x266_amd/csrc/x266_args.hpp (entropy_stats_levels, entropy_stats_side) against the contract as
tests/cpp/entropy_stats_rules_check.cpp writes it down -- single perturbations of a base tuple: NULL, alignment halves, saturating extents,
every illegal overlap, the rows of d_part, d_kind without d_mode, qp at -1 and 52, chroma_qp_offset at -13 and 13, no unit at all.  The same
driver runs the table rule and the counting sink under the two syntax walks against literals.  The driver is a stand-alone program, built
twice: plain, and with the address and undefined-behaviour sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest

import _cpp_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xEntropyStatsLevelsGpu", "xEntropyStatsSideGpu")
STRUCTS = ("x266_entropy_stats_t", "x266_entropy_side_stats_t")
HELPERS = ("xEntropyStatsRows", "xEntropyInitFromCounts", "xEntropyCountRegion", "xEntropyCountSideCtu")
DRIVER = "entropy_stats_rules_check"
CHECK_FLOOR = 1500                                                        # a walk that shrank must not pass quietly


@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="entropy_stats_rules_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared code compiles without a warning as plain C++
        return _cpp_driver.run(exe)


def driver_fields(call):
    """{field: (alignment, optional, output)} from the driver's line of the call, fields in printed order"""
    items = re.search(r"^%s: (.*)$" % call, driver_output(), re.M).group(1)
    got = {}
    for item in items.split(", "):
        m = re.fullmatch(r"(d_\w+) (\d+) (opt )?(in|out)", item)
        assert m, item
        got[m.group(1)] = (int(m.group(2)), bool(m.group(3)), m.group(4) == "out")
    return got


@_cpp_driver.needs_gxx
def test_the_rules_hold():
    text = driver_output()
    assert int(re.search(r"^checks entropy statistics (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR
    assert "sizeof(x266_entropy_stats_t) 48" in text and "sizeof(x266_entropy_side_stats_t) 72" in text


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment; the driver's
    line of each call names the fields of the struct in struct order at that alignment, optional where the comment says "or NULL" """
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    want = ({"d_level": 16, "d_class": 1, "d_nnz": 4, "d_counts": 8, "d_part": 16},
            {"d_kind": 1, "d_mode": 1, "d_class": 1, "d_qp": 1, "d_nnz": 4, "d_counts": 8, "d_part": 16})
    for call, struct, aligns in zip(CALLS, STRUCTS, want):
        stated = _cpp_driver.header_struct_fields(struct)
        assert {f: v[0] for f, v in stated.items()} == aligns and list(stated) == list(aligns)
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const %s \*p, void \*stream\);" % (call, struct), hdr)
        held = driver_fields(call)
        assert list(held) == list(stated)
        for field, (align, optional, output) in held.items():
            assert align == stated[field][0] and optional == stated[field][1] and output == (field in ("d_counts", "d_part")), (call, field)
    text = hdr[hdr.index("---- per-context bin statistics on the device"):hdr.index("#define X266_ENTROPY_STATS_REGIONS")]
    for said in ("(4096 z + n) / (2 n)", "rounded half up", "31 .. 2017", "2^51", "ADDS", "coded == 0", "canonical form", "bins[0]", "contract, not", "3456", "110 592",
                 "xEntropyStatsRows", "two launches", "no global\n * atomics", "captured into a graph", "read no launch option", "n == 0", "ballots and popcounts",
                 "one lane per CTU", "d_kind without d_mode", "the motion coder", "3 473", "1 947 of 2 040", "Backward\n * adaptation"):
        assert said in text, said
    # the two coders' blocks no longer list what this lands as missing, and still list the carry-over
    levels = hdr[hdr.index("---- the entropy coder:"):hdr.index("typedef struct x266_entropy_region_t")]
    side = hdr[hdr.index("---- the entropy coder of the side information"):hdr.index("#define X266_ENTROPY_SIDE_CONTEXTS")]
    assert "statistics coming" not in levels and "tables coming back" not in side and "carry-over" in levels and "carry-over" in side
    assert "xEntropyStatsLevelsGpu" in levels and "xEntropyStatsSideGpu" in side
    # "entropy" only behind xEntropy
    names = re.findall(r"\b(x[A-Z]\w*)\s*\(", hdr[hdr.index("#define X266_ENTROPY_STATS_REGIONS"):hdr.index("---- frame quality")])
    assert set(names) == set(CALLS + HELPERS)


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    import x266_amd.entropy as X
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + HELPERS:
        assert name in exported and hasattr(lib, name), name
    assert not [n for n in exported if "entropy" in n.lower() and not n.startswith("xEntropy")]
    p = X.entropy_stats_params(d_level=0x1000, d_counts=0x3000, n_regions=7)
    assert (p.d_level, p.d_class, p.d_nnz, p.d_counts, p.d_part, p.n_regions) == (0x1000, None, None, 0x3000, None, 7)
    q = X.entropy_side_stats_params(d_kind=0x1000, d_counts=0x3000, n_ctu=7, qp=33, chroma_qp_offset=-4)
    assert (q.d_kind, q.d_mode, q.d_class, q.d_qp, q.d_nnz, q.d_counts, q.d_part, q.n_ctu, q.qp, q.chroma_qp_offset) == (0x1000, None, None, None, None, 0x3000, None, 7, 33, -4)
    for call, params, struct in zip(CALLS, (p, q), (x266_amd.EntropyStatsParams, x266_amd.EntropySideStatsParams)):
        fn = getattr(lib, call)
        assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(struct)
        assert fn(None, ctypes.byref(params), None) == -1                     # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1                                     # ... and so is a NULL p
    P, Q = x266_amd.EntropyStatsParams, x266_amd.EntropySideStatsParams
    assert ctypes.sizeof(P) == 48 and P.d_counts.offset == 24 and P.d_part.offset == 32 and P.n_regions.offset == 40
    assert ctypes.sizeof(Q) == 72 and Q.d_counts.offset == 40 and Q.d_part.offset == 48 and Q.n_ctu.offset == 56 and Q.qp.offset == 64 and Q.chroma_qp_offset.offset == 68
    assert x266_amd.ENTROPY_STATS_REGIONS == 32 and x266_amd.ENTROPY_SIDE_STATS_CTUS == 64


def test_the_binding_and_the_one_copy_of_each_syntax():
    """the keyword builders refuse an unknown field; the calls are module functions and Codec gains none.  The statistics add no second
    copy of either syntax: the walks are templates over their sink, the host helpers and the side kernel run them with the counting sink,
    and the level kernel is a data-parallel statement with no serial section; two launches per call, no atomics, no wait"""
    import x266_amd
    import x266_amd.entropy as X
    with pytest.raises(TypeError) as e:
        X.entropy_stats_params(bogus=1, d_level=16)
    assert str(e.value) == "entropy_stats_params: no such field: ['bogus']"
    with pytest.raises(TypeError):
        X.entropy_side_stats_params(d_stream=16)
    for name in ("entropy_stats_params", "entropy_side_stats_params", "entropy_stats_levels", "entropy_stats_levels_dev", "entropy_stats_side", "entropy_stats_side_dev",
                 "entropy_init_from_counts", "entropy_count_region", "entropy_count_side_ctu", "entropy_stats_rows"):
        assert callable(getattr(X, name)), name
    assert not [n for n in dir(x266_amd.Codec) if "stats_levels" in n or "stats_side" in n or "from_counts" in n]
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, levels_syntax, side_syntax, abi, driver, makefile = (open(os.path.join(*n)).read() for n in (
        (csrc, "entropy_stats_kernels.hip"), (csrc, "x266_entropy.hpp"), (csrc, "x266_entropy_side.hpp"), (csrc, "x266hip_abi.hip"),
        (ROOT, "tests", "cpp", DRIVER + ".cpp"), (csrc, "Makefile")))
    assert "entropy_stats_kernels.hip" in makefile
    for name, home in (("entropy_encode_region", "x266_entropy.hpp"), ("entropy_side_encode_ctu", "x266_entropy_side.hpp")):
        text = levels_syntax if home == "x266_entropy.hpp" else side_syntax
        assert len(re.findall(r"template <class Sink>\s*X266_HD inline void %s\(Sink &e," % name, text)) == 1, name
        for other in os.listdir(csrc):                                       # one copy of each walk in the whole library
            if other.endswith((".hpp", ".hip", ".cpp")):
                copies = len(re.findall(r"inline \w+ %s\(" % name, open(os.path.join(csrc, other)).read()))
                assert copies == (1 if other == home else 0), (name, other)
        assert "EntropyCounter<uint64_t, 1>" in abi and name + "(e," in abi and name + "(e," in driver
    assert "struct EntropyCounter" in levels_syntax and "struct EntropyCounter" not in side_syntax and "struct EntropyCounter" not in kernel
    assert "entropy_side_encode_ctu(e," in kernel and "EntropyCounter<uint32_t, 64>" in kernel
    assert "entropy_encode_region" not in kernel and "EntropyEnc" not in kernel             # the level kernel is not the coder's walk
    assert not re.search(r"atomic(Add|Min|Max|CAS|Exch)|__hip_atomic|while\s*\(|hipLaunchCooperative|hipMalloc|hipStreamSynchronize|hipDeviceSynchronize", kernel)
    assert kernel.count("hipLaunchKernelGGL(") == 4                         # per call: the rows, then the totals
    assert "__ballot(" in kernel and "__popc(" in kernel and "wave_sum(" in kernel
    # the encoders' kernel files are as they were: their tests count launches and copies there
    for name, launches in (("entropy_kernels.hip", 4), ("entropy_motion_kernels.hip", 5), ("entropy_side_kernels.hip", 4)):
        assert open(os.path.join(csrc, name)).read().count("hipLaunchKernelGGL(") == launches
