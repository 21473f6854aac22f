"""CPU: the surface and the argument rules of xEntropyEncodeSideGpu and xEntropyDecodeSideGpu: header, struct layout, exports, bindings,
and the rule functions of x266_amd/csrc/x266_args.hpp (entropy_side_encode, entropy_side_decode) against the contract as
tests/cpp/entropy_side_rules_check.cpp writes it down -- single perturbations of a base tuple: alignment halves, saturating extents, every
illegal overlap, a NULL d_stream with a capacity, d_kind without d_mode, an entry of init at 30 and at 2018, qp at -1 and 52,
chroma_qp_offset at -13 and 13.  The same driver runs the syntax of x266_amd/csrc/x266_entropy_side.hpp against the header's worked
values.  The driver is a stand-alone program, built twice: plain, and with the address and undefined-behaviour sanitizers.  g++ only: no
GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest

import _cpp_driver
import _entropy_side_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xEntropyEncodeSideGpu", "xEntropyDecodeSideGpu")
HELPERS = ("xEntropySideDefaultInit", "xEntropyEncodeSideCtu", "xEntropyDecodeSideCtu")
DRIVER = "entropy_side_rules_check"
ARRAYS = ["d_kind", "d_mode", "d_class", "d_qp", "d_nnz"]
CHECK_FLOOR = 7000                                                        # a walk that shrank must not pass quietly


@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="entropy_side_rules_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared syntax compiles without a warning as plain C++
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
    assert int(re.search(r"^checks x266_entropy_side_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR
    assert "sizeof(x266_entropy_side_ctu_t) 32" in text and "sizeof(x266_entropy_side_t) 104" in text


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment; the driver's
    line of each call names fields of the struct in struct order at that alignment, optional where the comment says "or NULL" """
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    stated = _cpp_driver.header_struct_fields("x266_entropy_side_t")
    assert list(stated) == ARRAYS + ["d_coded", "d_stream", "d_total", "d_status"]
    assert {f: v[0] for f, v in stated.items()} == {"d_kind": 1, "d_mode": 1, "d_class": 1, "d_qp": 1, "d_nnz": 4, "d_coded": 8, "d_stream": 16, "d_total": 8,
                                                    "d_status": 1}
    for call in CALLS:
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_entropy_side_t \*p, void \*stream\);" % call, hdr)
        held = driver_fields(call)
        assert list(held) == [f for f in stated if f in held]
        for field, (align, optional, _) in held.items():
            assert align == stated[field][0] and optional == stated[field][1], (call, field)
    assert list(driver_fields(CALLS[0])) == list(stated)[:8] and list(driver_fields(CALLS[1])) == [f for f in stated if f != "d_total"]
    assert {f for f, v in driver_fields(CALLS[0]).items() if v[2]} == {"d_coded", "d_stream", "d_total"}
    assert {f for f, v in driver_fields(CALLS[1]).items() if v[2]} == set(ARRAYS) | {"d_status"}
    body = re.search(r"typedef struct x266_entropy_side_ctu_t \{(.*?)\} x266_entropy_side_ctu_t;", hdr, re.S).group(1)
    assert re.findall(r"\buint(?:32|64)_t\s+(\w+);", body) == ["ctx_bins", "bypass_bins", "offset", "n_words", "n_bytes", "n_intra", "n_coded"]
    text = hdr[hdr.index("---- the entropy coder of the side information"):hdr.index("#define X266_ENTROPY_SIDE_CONTEXTS")]
    for said in ("r = 6 ctu + q", "Canonical values", "ONE chroma kind", "X266_TDECIDE_CLASSES", "most probable modes", "Truncated unary", "Exp-Golomb order 0",
                 "more than 5 ones", "flat CTU", "0 bytes", "Round trip", "31 .. 2017", "under 485 bits", "65 bytes", "Worked values", "count-only", "ONE LANE per CTU",
                 "Every loop is bounded", "d_kind without d_mode", "Out of scope", "B-frames", "SAO and ALF", "container", "carry-over", "class_bits", "adapted tables"):
        assert said in text, said
    # the two older blocks and the README point here, and what they said was missing is no longer listed as missing
    levels = hdr[hdr.index("---- the entropy coder:"):hdr.index("typedef struct x266_entropy_region_t")]
    motion = hdr[hdr.index("---- the entropy coder of the motion stream"):hdr.index("#define X266_ENTROPY_MOTION_CONTEXTS")]
    assert "xEntropyEncodeSideGpu" in levels and "xEntropyEncodeSideGpu" in motion and "Until the side information is coded" not in levels
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "xEntropyEncodeSideGpu" in readme and "classes, modes, kinds and qp are still uncoded" in readme and "would still leave the class bytes uncoded" not in readme
    # no exported name holds "motion", and "entropy" only behind xEntropy
    names = re.findall(r"\b(x[A-Z]\w*Side\w*)\s*\(", text + hdr[hdr.index("#define X266_ENTROPY_SIDE_CONTEXTS"):hdr.index("---- frame quality")])
    assert set(CALLS + HELPERS) <= set(names) and all(n.startswith("xEntropy") and "otion" not in n for n in names)


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
    for call in CALLS:
        fn = getattr(lib, call)
        assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.EntropySideParams)
        p = X.entropy_side_params(d_kind=0x1000, d_coded=0x3000, init=0x5000, n_ctu=7, cap_words=5, qp=33, chroma_qp_offset=-4)
        assert (p.d_kind, p.d_mode, p.d_class, p.d_qp, p.d_nnz, p.d_coded, p.d_stream, p.d_total, p.d_status, p.init) == \
            (0x1000, None, None, None, None, 0x3000, None, None, None, 0x5000)
        assert (p.n_ctu, p.cap_words, p.qp, p.chroma_qp_offset) == (7, 5, 33, -4)
        assert fn(None, ctypes.byref(p), None) == -1                          # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1                                     # ... and so is a NULL p
    P = x266_amd.EntropySideParams
    assert ctypes.sizeof(P) == 104 and P.d_nnz.offset == 32 and P.init.offset == 72 and P.n_ctu.offset == 80 and P.cap_words.offset == 88
    assert P.qp.offset == 96 and P.chroma_qp_offset.offset == 100
    assert x266_amd.ENTROPY_SIDE_CTU_DTYPE.itemsize == 32 and x266_amd.ENTROPY_SIDE_CTU_DTYPE == S.CODED_DTYPE
    assert x266_amd.ENTROPY_SIDE_CONTEXTS == S.CONTEXTS == 16 and x266_amd.ENTROPY_SIDE_MAX_BYTES == S.MAX_BYTES == 80


def test_the_binding_and_the_one_copy_of_the_syntax():
    """entropy_side_params refuses an unknown field in the keyword builders' words; the calls are module functions and Codec has none of
    them.  The kernels, the rules driver and the host helpers take the syntax from x266_entropy_side.hpp and the coder from
    x266_entropy.hpp, which is not copied; the offset scan is the one kernel of the level stream; the kernels neither wait nor count"""
    import x266_amd
    import x266_amd.entropy as X
    with pytest.raises(TypeError) as e:
        X.entropy_side_params(bogus=1, d_kind=16)
    assert str(e.value) == "entropy_side_params: no such field: ['bogus']"
    for name in ("entropy_side_params", "entropy_encode_side", "entropy_decode_side", "entropy_encode_side_dev", "entropy_decode_side_dev",
                 "entropy_side_default_init", "entropy_encode_side_ctu", "entropy_decode_side_ctu"):
        assert callable(getattr(X, name)), name
    assert not [n for n in dir(x266_amd.Codec) if "entropy_side" in n or "encode_side" in n or "decode_side" in n]
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, syntax, coder, levels_h, abi, driver, makefile = (open(os.path.join(*n)).read() for n in (
        (csrc, "entropy_side_kernels.hip"), (csrc, "x266_entropy_side.hpp"), (csrc, "x266_entropy.hpp"), (csrc, "x266_levels.hpp"), (csrc, "x266hip_abi.hip"),
        (ROOT, "tests", "cpp", DRIVER + ".cpp"), (csrc, "Makefile")))
    for text in (kernel, abi, driver):
        assert '#include "x266_entropy_side.hpp"' in text
    assert '#include "x266_entropy.hpp"' in syntax and "entropy_side_kernels.hip" in makefile and "x266_entropy_side.hpp" in makefile
    for name in ("entropy_side_encode_ctu", "entropy_side_decode_ctu", "entropy_side_flat_ctu", "entropy_side_canon"):
        assert len(re.findall(r"inline \w+ %s\(" % name, syntax)) == 1 and name + "(" in kernel and name + "(" in abi and name + "(" in driver, name
        for other in os.listdir(csrc):                                       # the syntax appears once, in the new header
            if other != "x266_entropy_side.hpp" and other.endswith((".hpp", ".hip", ".cpp")):
                assert not re.search(r"inline \w+ %s\(" % name, open(os.path.join(csrc, other)).read()), (name, other)
    for name in ("entropy_side_mpm", "entropy_side_chroma_list"):
        assert len(re.findall(r"inline \w+ %s\(" % name, syntax)) == 1 and name + "(" not in kernel and name + "(" not in abi
    for name in ("entropy_enc_bin", "entropy_enc_bypass", "entropy_enc_bits", "entropy_dec_bin", "entropy_dec_bypass", "entropy_dec_bits"):
        assert re.search(r"inline \w+ %s\(" % name, coder) and name + "(" in syntax and not re.search(r"inline \w+ %s\(" % name, syntax), name
    assert "struct EntropyEnc" not in syntax and "struct EntropyDec" not in syntax and "entropy_shift_low" not in syntax
    assert "struct EntropyEnc" not in kernel and "entropy_shift_low" not in kernel
    assert len(re.findall(r"void levels_scan_kernel\(", levels_h)) == 1 and "levels_scan_kernel<x266_entropy_side_ctu_t>" in kernel
    assert not re.search(r"atomic(Add|Min|Max|CAS|Exch)|__hip_atomic|while\s*\(|hipLaunchCooperative|__syncthreads", kernel)   # no atomics, no wait of any kind
    assert not re.search(r"\bdo\b|while\s*\(|for\s*\(\s*;\s*;", syntax)                                                       # bounded trip counts only
    assert kernel.count("hipLaunchKernelGGL(") == 4                         # encode: count, scan, write; decode: one
    assert "stride" in syntax and "kSideCtxStride" in kernel and "1u, qp" in abi                       # the contexts through a stride: 1 on the host
    # the two older kernel files are as they were: their tests count launches and copies there
    for name, launches in (("entropy_kernels.hip", 4), ("entropy_motion_kernels.hip", 5)):
        text = open(os.path.join(csrc, name)).read()
        assert text.count("hipLaunchKernelGGL(") == launches and text.count("substream_copy(") == 2 and "entropy_side" not in text
