"""CPU: the surface and the argument rules of xEntropyEncodeMvGpu, xEntropyDecodeMvGpu and xMotionReconstructGpu: header, struct layout,
exports, bindings, and the rule functions of x266_amd/csrc/x266_args.hpp (entropy_motion_encode, entropy_motion_decode, motion_reconstruct)
against the contract as tests/cpp/entropy_motion_rules_check.cpp writes it down -- single perturbations of a base tuple: alignment halves,
saturating extents, every illegal overlap, a NULL d_stream or d_words with a non-zero count, an entry of init at 30 and at 2018, sides that
are no multiple of 16.  The same driver runs the syntax of x266_amd/csrc/x266_entropy_motion.hpp against the header's worked values.  The
driver is a stand-alone program, built twice: plain, and with the address and undefined-behaviour sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest

import _cpp_driver
import _entropy_motion_ref as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xEntropyEncodeMvGpu", "xEntropyDecodeMvGpu")
RECON = "xMotionReconstructGpu"
HELPERS = ("xEntropyMvDefaultInit", "xEntropyEncodeMvCtu", "xEntropyDecodeMvCtu")
DRIVER = "entropy_motion_rules_check"
CHECK_FLOOR = 2500                                                        # a walk that shrank must not pass quietly


@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="entropy_motion_rules_") as where:
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
    assert int(re.search(r"^checks x266_entropy_motion_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR
    assert "sizeof(x266_entropy_motion_ctu_t) 32" in text and "sizeof(x266_entropy_motion_t) 80" in text


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment; the driver's
    line of each call names fields of the struct in struct order at that alignment, optional where the comment says "or NULL" """
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    stated = _cpp_driver.header_struct_fields("x266_entropy_motion_t")
    assert list(stated) == ["d_ctu", "d_words", "d_coded", "d_stream", "d_total", "d_status"]
    assert {f: v[0] for f, v in stated.items()} == {"d_ctu": 8, "d_words": 16, "d_coded": 8, "d_stream": 16, "d_total": 8, "d_status": 1}
    for call in CALLS:
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_entropy_motion_t \*p, void \*stream\);" % call, hdr)
        held = driver_fields(call)
        assert list(held) == [f for f in stated if f in held]
        for field, (align, optional, _) in held.items():
            assert align == stated[field][0] and optional == stated[field][1], (call, field)
    assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_motion_t \*p, void \*stream\);" % RECON, hdr)
    assert list(driver_fields(CALLS[0])) == list(stated)[:5] and list(driver_fields(CALLS[1])) == [f for f in stated if f != "d_total"]
    assert {f for f, v in driver_fields(CALLS[0]).items() if v[2]} == {"d_coded", "d_stream", "d_total"}
    assert {f for f, v in driver_fields(CALLS[1]).items() if v[2]} == {"d_ctu", "d_words", "d_status"}
    body = re.search(r"typedef struct x266_entropy_motion_ctu_t \{(.*?)\} x266_entropy_motion_ctu_t;", hdr, re.S).group(1)
    assert re.findall(r"\buint(?:32|64)_t\s+(\w+);", body) == ["ctx_bins", "bypass_bins", "offset", "n_words", "n_bytes", "parts", "unreadable"]
    text = hdr[hdr.index("---- the entropy coder of the motion stream"):hdr.index("#define X266_ENTROPY_MOTION_CONTEXTS")]
    for said in ("split[k]", "TRUE differences", "Exp-Golomb order 1", "more than 14 ones", "FLAT CTU", "unreadable = 1", "31 .. 2017", "5645 bits", "710 bytes",
                 "511 bytes", "Worked values", "count-only", "256 c", "cx + 2 cy", "never read", "Out of scope", "carry-over", "== x266_motion_ctu_t.bits exactly"):
        assert said in text, said
    # the two older blocks point here instead of listing the calls as missing
    motion = hdr[hdr.index("compact motion stream"):hdr.index("typedef struct x266_motion_ctu_t")]
    assert "xMotionReconstructGpu" in motion and "xEntropyEncodeMvGpu" in motion and "it needs a wavefront" not in motion
    levels = hdr[hdr.index("---- the entropy coder:"):hdr.index("typedef struct x266_entropy_region_t")]
    assert "xEntropyEncodeMvGpu" in levels and "follow-ups: coding the motion stream" not in levels
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "classes, modes, kinds and qp are still uncoded" in readme and "classes, modes, qp, motion -- is still uncoded" not in readme


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    import x266_amd.entropy as X
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + HELPERS + (RECON,):
        assert name in exported and hasattr(lib, name), name
    for call in CALLS:
        fn = getattr(lib, call)
        assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.EntropyMotionParams)
        p = X.entropy_motion_params(d_ctu=0x1000, d_coded=0x3000, init=0x5000, width=144, height=112, in_words=9, cap_words=5)
        assert (p.d_ctu, p.d_words, p.d_coded, p.d_stream, p.d_total, p.d_status, p.init) == (0x1000, None, 0x3000, None, None, None, 0x5000)
        assert (p.width, p.height, p.in_words, p.cap_words) == (144, 112, 9, 5)
        assert fn(None, ctypes.byref(p), None) == -1                          # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1                                     # ... and so is a NULL p
    assert getattr(lib, RECON)(None, None, None) == -1
    P = x266_amd.EntropyMotionParams
    assert ctypes.sizeof(P) == 80 and P.init.offset == 48 and P.width.offset == 56 and P.in_words.offset == 64 and P.cap_words.offset == 72
    assert x266_amd.ENTROPY_MOTION_CTU_DTYPE.itemsize == 32 and x266_amd.ENTROPY_MOTION_CTU_DTYPE == EM.CODED_DTYPE


def test_the_binding_and_the_one_copy_of_the_syntax():
    """entropy_motion_params refuses an unknown field in the keyword builders' words; the calls are module functions.  The kernels, the
    rules driver and the host helpers take the syntax from x266_entropy_motion.hpp and the coder from x266_entropy.hpp, which is not copied;
    the slab copy is one function for both coders; the offset scan is one kernel for the four streams; reconstruct walks by stream order"""
    import x266_amd.entropy as X
    import x266_amd.motion as XM
    with pytest.raises(TypeError) as e:
        X.entropy_motion_params(bogus=1, d_ctu=16)
    assert str(e.value) == "entropy_motion_params: no such field: ['bogus']"
    for name in ("entropy_motion_params", "entropy_encode_motion", "entropy_decode_motion", "entropy_encode_motion_dev", "entropy_decode_motion_dev",
                 "entropy_motion_default_init", "entropy_encode_motion_ctu", "entropy_decode_motion_ctu"):
        assert callable(getattr(X, name)), name
    assert callable(XM.motion_reconstruct)
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, syntax, coder, levels_kernel, levels_h, abi, motion_h = (open(os.path.join(csrc, n)).read() for n in (
        "entropy_motion_kernels.hip", "x266_entropy_motion.hpp", "x266_entropy.hpp", "entropy_kernels.hip", "x266_levels.hpp", "x266hip_abi.hip", "x266_motion.hpp"))
    assert '#include "x266_entropy_motion.hpp"' in kernel and '#include "x266_entropy_motion.hpp"' in abi and '#include "x266_entropy.hpp"' in syntax
    for name in ("entropy_motion_encode_ctu", "entropy_motion_decode_ctu", "entropy_motion_flat_ctu"):
        assert re.search(r"inline \w+ %s\(" % name, syntax) and name + "(" in kernel and name + "(" in abi, name
    for name in ("entropy_enc_bin", "entropy_enc_bypass", "entropy_enc_bits", "entropy_dec_bin", "entropy_dec_bypass", "entropy_dec_bits"):
        assert re.search(r"inline \w+ %s\(" % name, coder) and name + "(" in syntax and not re.search(r"inline \w+ %s\(" % name, syntax), name
    assert "struct EntropyEnc" not in syntax and "struct EntropyDec" not in syntax and "entropy_shift_low" not in syntax
    assert len(re.findall(r"void substream_copy\(", coder)) == 1 and "void substream_copy" not in kernel + levels_kernel
    assert kernel.count("substream_copy(") == 2 and levels_kernel.count("substream_copy(") == 2
    assert len(re.findall(r"void levels_scan_kernel\(", levels_h)) == 1 and "levels_scan_kernel<x266_entropy_motion_ctu_t>" in kernel
    assert "motion_predictor_from(" in kernel and re.search(r"inline PartVec motion_predictor_from\(", motion_h)
    assert not re.search(r"atomic(Add|Min|Max|CAS|Exch)|__hip_atomic|while\s*\(|hipLaunchCooperative", kernel)      # no atomics, no spin-wait
    assert not re.search(r"\bdo\b|while\s*\(\s*(1|true)\s*\)|for\s*\(\s*;\s*;", syntax)                                # bounded trip counts only
    assert kernel.count("hipLaunchKernelGGL(") == 5                         # encode: count, scan, write; decode: one; reconstruct: one per step
    assert "count <= 14" not in coder
